"""Raw kernel launchers: torch tensors in (device memory + stream plumbing only), libmico_hip.so C-ABI calls out.

No autograd here and no fallback: every function requires CUDA(HIP) tensors and raises MicoHipError otherwise.
All launches go to torch's current stream.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import F16, BF16, F32, ACT_NONE, ACT_GELU, ACT_GELU_GRAD, ACT_GELU_SAVE_DERIV, ACT_MUL_AUX, GemmEpilogue, AttnParams, MicoHipError, check

_DT = {torch.float16: F16, torch.bfloat16: BF16, torch.float32: F32}


def dt_code(dtype):
    return _DT[dtype]


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise MicoHipError("mico_amd kernels need device tensors (got a CPU tensor); there is no CPU fallback")
    return t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional per-launch HIP-event timing of the GEMM kernel (bench.py's roofline leg).  Events are recorded on the
    stream the kernel is launched on (torch's current stream)."""

    def __init__(self, variants=((0, 0), (0, 1), (1, 1))):
        self.variants = set(variants)
        self.records = []   # ((ta, tb, kernel), flops, start_event, end_event); kernel: 0 small tile, 1 8-wave, 2 producer/consumer
        self.detail = []    # per record: (M, N, K, epilogue signature) - bench.py --gemm-detail

    def summary(self):
        out = {}
        for var, flops, e0, e1 in self.records:
            d = out.setdefault(var, dict(launches=0, flops=0.0, ms=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["ms"] += e0.elapsed_time(e1)
        return out


GEMM_TIMER = None


def pad8(n):
    return (n + 7) // 8 * 8


_SPLITK_WS = {}
SPLITK_WS_STREAMS = 4   # scratch buffers kept: the most recently used (device, stream) pairs
SPLITK_SLABS = True   # False: weight-gradient launches get no scratch and fall back to fp32 atomics (kept tested: the C-ABI makes the scratch optional)
SPLITK_WS_CAP = 320 << 20   # bytes: room for 8+ slabs of the towers' largest layer gradient (6144 x 1408 fp32 = 35 MB); a smaller scratch only
                            # bounds the split count (the library falls back to fewer splits / atomics cleanly)


def _splitk_scratch(nbytes, device):
    """One fp32 scratch buffer per (device, stream), grown on demand and kept.  The weight-gradient kernel writes its split-K partial
    tiles into it and the reduction pass reads them back: launches on ONE stream use it one after the other; launches on different
    streams (or from threads with different current streams) must not share it - hence the stream in the key."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    t = _SPLITK_WS.pop(key, None)
    if t is None or t.numel() * 4 < nbytes:
        t = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    _SPLITK_WS[key] = t                          # (re-inserted last: the dict is the LRU order)
    while len(_SPLITK_WS) > SPLITK_WS_STREAMS:   # streams created per step would otherwise each pin up to SPLITK_WS_CAP bytes for ever
        _SPLITK_WS.pop(next(iter(_SPLITK_WS)))
    return t


def release_scratch():
    """Drop the cached split-K scratch buffers (runtime.reset())."""
    _SPLITK_WS.clear()


def gemm(A, B, out, *, ta=False, tb=False, M=None, N=None, K=None, bias=None, aux_out=None, aux_in=None, act=ACT_NONE,
         row_scale=None, rows_per_scale=0, resid=None, pos=None, pos_rows=0, remap=(0, 0, 0), alpha=1.0,
         accumulate=False, split_k=1, dtype=None, ksegs=None, row_map=None, rows_per_map=0, drop=None, colsum_out=None, aux_tiled=False):
    """out = epilogue(opA(A) @ opB(B)); see include/mico_hip.h (mico_gemm).  A/B are 2-D 16-bit tensors (row stride =
    leading dim).  ta: A stored [K,M]; tb: B stored [K,N].  aux_tiled: the aux tensor is an AuxTiled-sized buffer in the MLP pair's
    private layout (mico_gemm_epilogue::aux_tiled; aux_buffer() below decides)."""
    dtype = dtype or A.dtype
    if A.dtype != B.dtype:   # the kernel takes ONE element type for both operands: mixed bit patterns would multiply silently
        raise MicoHipError(f"mico_gemm operands differ in dtype ({A.dtype} x {B.dtype}): a backward pass running under another "
                           "runtime.precision than its forward?")
    if M is None:
        M = A.shape[1] if ta else A.shape[0]
    if K is None:
        K = A.shape[0] if ta else A.shape[1]
    if N is None:
        N = B.shape[1] if tb else B.shape[0]
    e = GemmEpilogue()
    e.bias = _p(bias)
    e.aux_out = _p(aux_out)
    e.aux_in = _p(aux_in)
    aux = aux_out if aux_out is not None else aux_in
    e.ldaux = aux.stride(0) if aux is not None else 0
    if aux_out is not None and aux_in is not None:
        # GELU_GRAD with both (the pre-activation-keeping MLP pair): aux_in = the pre-activation (tiled with aux_tiled), aux_out = gelu(aux_in), always
        # row-major; one leading dimension serves both
        if act != ACT_GELU_GRAD or (not aux_tiled and aux_in.stride(0) != aux_out.stride(0)):
            raise MicoHipError("mico_gemm: aux_in together with aux_out is the GELU_GRAD launch that also writes gelu(aux_in); both row-major tensors share ldaux")
    if aux_tiled:
        _check_tiled(aux_in if aux_in is not None else aux, M, N)
        e.aux_tiled = 1
        if aux_out is None or aux_in is None:
            e.ldaux = N
    e.act = act
    e.row_scale = _p(row_scale)
    e.rows_per_scale = rows_per_scale
    e.resid = _p(resid)
    e.pos = _p(pos)
    e.pos_rows = pos_rows
    e.remap_group, e.remap_skip, e.remap_offset = remap
    e.alpha = alpha
    e.accumulate = 1 if accumulate else 0
    e.row_map = _p(row_map)
    e.rows_per_map = rows_per_map
    if drop is not None:   # (p, seed, site)
        e.drop_p, e.drop_seed, e.drop_site = float(drop[0]), int(drop[1]) & 0xFFFFFFFF, int(drop[2])
    e.colsum_out = _p(colsum_out)
    if SPLITK_SLABS and accumulate and out.dtype == torch.float32 and split_k != 1 and ta and tb:
        # scratch for the split-K slabs of the weight-gradient kernels (mico_gemm_epilogue::splitk_ws): room for 8 splits of the towers'
        # large layers, 32 of BERT's small ones
        slab = M * N * 4
        ws = _splitk_scratch(min(32, max(2, SPLITK_WS_CAP // slab)) * slab, out.device)
        e.splitk_ws, e.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4
    if ksegs is not None:   # (kseg, a_offsets, b_offsets)
        e.kseg, e.nseg = ksegs[0], len(ksegs[1])
        for i, (ao, bo) in enumerate(zip(ksegs[1], ksegs[2])):
            e.a_seg_off[i], e.b_seg_off[i] = ao, bo
        K = e.kseg * e.nseg
    timer = GEMM_TIMER
    timed = timer is not None and (int(ta), int(tb)) in timer.variants
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = _lib.lib().mico_gemm(int(ta), int(tb), M, N, K, _p(A), A.stride(0), _p(B), B.stride(0), _p(out), out.stride(0),
                              dt_code(out.dtype), C.byref(e), split_k, dt_code(dtype), _st())
    if timed:
        e1.record()
        timer.records.append(((int(ta), int(tb), int(_lib.lib().mico_gemm_last_kernel())), 2.0 * M * N * K, e0, e1))
        sig = "".join(c for c, on in (("b", bias is not None), ("x", aux_out is not None), ("i", aux_in is not None), ("g", act != ACT_NONE),
                                      ("s", row_scale is not None), ("r", resid is not None), ("m", row_map is not None),
                                      ("a", accumulate), ("d", drop is not None), ("p", pos is not None)) if on)
        timer.detail.append((M, N, K, sig + ("/f32" if out.dtype == torch.float32 else ""), split_k))
    check(rc, "mico_gemm")
    return out


def _check_tiled(aux, M, N):
    need = ((M + 255) // 256) * 256 * N
    if aux is None or not aux.is_contiguous() or aux.numel() < need:
        raise MicoHipError(f"aux_tiled: the aux tensor of an [{M}, {N}] launch is a contiguous buffer of >= {need} elements (ops.aux_buffer)")


def aux_buffer(M, N, K, dtype, device, tiled_ok=True):
    """The tensor that carries gelu'(pre-activation) from an MLP's forward GEMM (GELU_SAVE_DERIV, aux_out) to its backward (MUL_AUX, aux_in):
    (buffer, tiled).  tiled = both launches - [M, N] over a reduction of K - run on the persistent 8-phase kernel, which keeps the tensor in its
    accumulator layout (mico_gemm_epilogue::aux_tiled; M rounded up to 256 rows); otherwise (or with tiled_ok = False: launches the caller
    knows to go elsewhere - fp8 mode, three k-segments) the documented row-major [M, N]."""
    n = int(_lib.lib().mico_gemm_aux_tiled_elems(M, N, K)) if (AUX_TILED and tiled_ok) else 0
    if n > 0:
        return torch.empty((n // N, N), dtype=dtype, device=device), True
    return torch.empty((M, N), dtype=dtype, device=device), False


AUX_TILED = os.environ.get("MICO_AUX_TILED", "1") != "0"     # A/B switch: 0 keeps every aux tensor row-major


def _epilogue(bias=None, aux_out=None, aux_in=None, act=ACT_NONE, row_scale=None, rows_per_scale=0, resid=None, pos=None, pos_rows=0,
              remap=(0, 0, 0), alpha=1.0, accumulate=False, row_map=None, rows_per_map=0, drop=None, aux_tiled=False, tiled_shape=None):
    e = GemmEpilogue()
    e.bias, e.aux_out, e.aux_in = _p(bias), _p(aux_out), _p(aux_in)
    aux = aux_out if aux_out is not None else aux_in
    e.ldaux = aux.stride(0) if aux is not None else 0
    if aux_tiled:
        _check_tiled(aux, *tiled_shape)
        e.aux_tiled, e.ldaux = 1, tiled_shape[1]
    e.act = act
    e.row_scale, e.rows_per_scale = _p(row_scale), rows_per_scale
    e.resid, e.pos, e.pos_rows = _p(resid), _p(pos), pos_rows
    e.remap_group, e.remap_skip, e.remap_offset = remap
    e.alpha = alpha
    e.accumulate = 1 if accumulate else 0
    e.row_map, e.rows_per_map = _p(row_map), rows_per_map
    if drop is not None:
        e.drop_p, e.drop_seed, e.drop_site = float(drop[0]), int(drop[1]) & 0xFFFFFFFF, int(drop[2])
    return e


class Mx8:
    """An MX-fp8 operand: q uint8 [rows, K] (OCP e4m3 bytes) + scales int32 [K / 128, rows] (four E8M0 bytes per word), see mico_quant_mx8."""
    __slots__ = ("q", "scales")

    def __init__(self, q, scales):
        self.q, self.scales = q, scales

    def dequant(self):
        """fp32 [rows, K] - tests and error measurements only."""
        rows, K = self.q.shape
        v = self.q.view(torch.float8_e4m3fn).float()
        w = self.scales.t().contiguous().view(torch.uint8).view(rows, K // 128, 4).reshape(rows, K // 32).float()
        return v * torch.exp2(w - 127.0).repeat_interleave(32, dim=1)


def quant_mx8(x, pre_scale=1.0, rows=None):
    """16-bit [rows, K] (row stride = ld) -> Mx8; K % 128 == 0."""
    rows = rows if rows is not None else x.shape[0]
    K = x.shape[1]
    q = torch.empty((rows, K), dtype=torch.uint8, device=x.device)
    sc = torch.empty((K // 128, rows), dtype=torch.int32, device=x.device)
    check(_lib.lib().mico_quant_mx8(_p(x), x.stride(0), rows, K, _p(q), q.stride(0), _p(sc), float(pre_scale), dt_code(x.dtype), _st()),
          "mico_quant_mx8")
    return Mx8(q, sc)


def gemm_mx8(A, B, out, *, dtype, M=None, **epi):
    """out = epilogue(A B^T) on the block-scaled fp8 MFMA; A [M, K] / B [N, K] Mx8 operands; dtype = the 16-bit type of a 16-bit out /
    aux tensors; epilogue keywords as ops.gemm (no split-K, no k-segments)."""
    M = M if M is not None else A.q.shape[0]
    N, K = B.q.shape
    e = _epilogue(tiled_shape=(M, N), **epi)
    timer = GEMM_TIMER
    timed = timer is not None and (0, 0) in timer.variants
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = _lib.lib().mico_gemm_mx8(M, N, K, _p(A.q), A.q.stride(0), _p(A.scales), _p(B.q), B.q.stride(0), _p(B.scales), _p(out), out.stride(0),
                                  dt_code(out.dtype), C.byref(e), dt_code(dtype), _st())
    if timed:
        e1.record()
        timer.records.append(((0, 0, 4), 2.0 * M * N * K, e0, e1))
        timer.detail.append((M, N, K, "mx8" + ("/f32" if out.dtype == torch.float32 else ""), 1))
    check(rc, "mico_gemm_mx8")
    return out


def layernorm_fwd(x, gamma, beta, eps, *, out16=None, out32=None, mean=None, rstd=None, post_add=None,
                  post_rows_per_group=0, post_groups=0, split16=False, dtype=torch.float16, frame_map=None,
                  rows_per_frame=0, x_copy=None, xhat16=None, x_normalized=False, drop=None, valid_cols=0, mx8=None):
    """split16: out16 is [rows, 2*cols] and receives [hi | lo] (split-precision GEMM operand).  frame_map (int32 [frames]):
    compacting gather of whole frames out of x; the number of rows is then len(frame_map) * rows_per_frame.
    xhat16 (fp16 [rows, cols]): receives the normalised gathered rows - the half-size replacement of x_copy for the backward;
    x_normalized: x IS such a buffer (y = x gamma + beta, no statistics).  mx8: an Mx8 whose q / scales receive the fp8 operand."""
    rows, cols = x.shape[0], x.shape[1]
    if frame_map is not None:
        rows = frame_map.shape[0] * rows_per_frame
    if xhat16 is not None:
        assert xhat16.dtype == torch.float16 and xhat16.is_contiguous() and tuple(xhat16.shape) == (rows, cols)
    if x_normalized:
        assert x.dtype == torch.float16 and x.is_contiguous()
    p = _lib.LnFwdParams(x=_p(x), x_dtype=dt_code(x.dtype), x_normalized=int(bool(x_normalized)), gamma=_p(gamma), beta=_p(beta), y16=_p(out16),
                         y32=_p(out32), mean=_p(mean), rstd=_p(rstd), rows=rows, cols=cols, eps=eps, post_add=_p(post_add),
                         post_rows_per_group=post_rows_per_group, post_groups=post_groups, y16_split=int(split16), frame_map=_p(frame_map),
                         rows_per_frame=rows_per_frame, x_copy=_p(x_copy), xhat16=_p(xhat16), drop_p=float(drop[0]) if drop else 0.0,
                         drop_seed=(int(drop[1]) & 0xFFFFFFFF) if drop else 0, drop_site=int(drop[2]) if drop else 0, valid_cols=int(valid_cols),
                         q8=_p(mx8.q) if mx8 is not None else None, ldq=mx8.q.stride(0) if mx8 is not None else 0,
                         scales=_p(mx8.scales) if mx8 is not None else None)
    check(_lib.lib().mico_layernorm_fwd(C.byref(p), dt_code(dtype), _st()), "mico_layernorm_fwd")


def layernorm_fwd_mx8(x, gamma, beta, eps, *, out16, mean, rstd, dtype, frame_map=None, rows_per_frame=0, x_copy=None, xhat16=None,
                      x_normalized=False):
    """layernorm_fwd whose 16-bit output is also quantised to the MX fp8 operand of gemm_mx8 (returns the Mx8; == quant_mx8(out16))."""
    rows, cols = x.shape[0], x.shape[1]
    if frame_map is not None:
        rows = frame_map.shape[0] * rows_per_frame
    q = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    sc = torch.empty((cols // 128, rows), dtype=torch.int32, device=x.device)
    mx = Mx8(q, sc)
    layernorm_fwd(x, gamma, beta, eps, out16=out16, mean=mean, rstd=rstd, dtype=dtype, frame_map=frame_map, rows_per_frame=rows_per_frame,
                  x_copy=x_copy, xhat16=xhat16, x_normalized=x_normalized, mx8=mx)
    return mx


def layernorm_bwd(dy, x, gamma, mean, rstd, *, dy_scale=1.0, dx_add=None, dx32=None, dx16=None, scale16=1.0, dgamma=None, dbeta=None,
                  grad_scale=1.0, dtype=torch.float16, frame_map=None, rows_per_frame=0, valid_cols=0, dx16_dst=None, dx16_frame_scale=None,
                  dx16_drop=None, x_normalized=False):
    """frame_map: dx_add / dx32 are the full stream, addressed through the frame scatter; dy / x / mean / rstd are compact.
    dx16_dst / dx16_frame_scale: dx16 is laid out for the next consumer's frame set (mico_layernorm_bwd in include/mico_hip.h).
    dx16_drop: (p, seed, site) - dx16 also carries that dropout's mask (the gradient side of a hidden-state dropout).
    x_normalized: x is the forward's fp16 xhat16 copy (mean may be None)."""
    dp, dseed, dsite = (float(dx16_drop[0]), int(dx16_drop[1]) & 0xFFFFFFFF, int(dx16_drop[2])) if dx16_drop is not None else (0.0, 0, 0)
    rows, cols = x.shape[0], x.shape[1]
    ws = None
    if dgamma is not None or dbeta is not None:
        nblk = _lib.lib().mico_layernorm_bwd_nblk(rows)
        ws = torch.empty(2 * nblk * cols, dtype=torch.float32, device=x.device)
    if x_normalized:
        assert x.dtype == torch.float16 and x.is_contiguous()
    p = _lib.LnBwdParams(dy=_p(dy), dy_dtype=dt_code(dy.dtype), dy_scale=dy_scale, x=_p(x), x_dtype=dt_code(x.dtype),
                         x_normalized=int(bool(x_normalized)), gamma=_p(gamma), mean=_p(mean), rstd=_p(rstd), dx_add=_p(dx_add), dx32=_p(dx32),
                         dx16=_p(dx16), scale16=scale16, dgamma=_p(dgamma), dbeta=_p(dbeta), grad_scale=grad_scale, ws=_p(ws), rows=rows,
                         cols=cols, frame_map=_p(frame_map), rows_per_frame=rows_per_frame, valid_cols=int(valid_cols), dx16_dst=_p(dx16_dst),
                         dx16_frame_scale=_p(dx16_frame_scale), dx16_drop_p=dp, dx16_drop_seed=dseed, dx16_drop_site=dsite)
    check(_lib.lib().mico_layernorm_bwd(C.byref(p), dt_code(dtype), _st()), "mico_layernorm_bwd")


def dropout_(x, drop):
    """In-place dropout of a 2-D fp32 / 16-bit tensor with the (p, seed, site) counter hash (see mico_dropout)."""
    rows, cols = x.shape
    check(_lib.lib().mico_dropout(_p(x), dt_code(x.dtype), rows, cols, x.stride(0), float(drop[0]), int(drop[1]) & 0xFFFFFFFF,
                                  int(drop[2]), _st()), "mico_dropout")
    return x


ATTN_SMALLQ_MAX = 80   # query rows of the one-pass short-query backward (SqCfg::QMAX in csrc/attention.hip; hd 64 only)


def attn_bwd_smallq_ok(B, H, Sq, Sk, hd, drop=None, batch0=0):
    """True when mico_attn_bwd takes its one-pass short-query kernel for this launch - the only kernel that implements
    mico_attn_params.dkv_accumulate.  The library's own condition (csrc/attention.hip, mico_attn_bwd), restated so that a caller that wants
    the two-launch ITM triplet backward can fall back to the one-launch form instead of running into the library's check."""
    import os
    if os.environ.get("MICO_ATTN_NOSMALLQ") is not None or hd != 64 or Sq > ATTN_SMALLQ_MAX:
        return False
    p = float(drop[0]) if drop else 0.0
    return p <= 0.0 or (B + batch0) * H * Sq * Sk <= 0xFFFFFFFF


def _attn_params(B, H, Sq, Sk, hd, q, k, v, o, scale, mask, q_strides, k_strides, v_strides, o_strides, drop=None, kv_batch_mod=0, batch0=0,
                 dkv_accumulate=False, kv_index=None):
    p = AttnParams()
    p.kv_batch_mod = int(kv_batch_mod)
    if kv_index is not None:
        if kv_index.dtype != torch.int32 or kv_index.dim() != 1 or kv_index.numel() != B or not kv_index.is_contiguous():
            raise MicoHipError(f"kv_index is a contiguous int32 [B = {B}] device tensor (got {kv_index.dtype} {tuple(kv_index.shape)})")
        p.kv_index = _p(kv_index)
    p.batch0, p.dkv_accumulate = int(batch0), int(bool(dkv_accumulate))
    if drop is not None:
        p.drop_p, p.drop_seed, p.drop_site = float(drop[0]), int(drop[1]) & 0xFFFFFFFF, int(drop[2])
    p.B, p.H, p.Sq, p.Sk, p.hd = B, H, Sq, Sk, hd
    p.q_bs, p.q_rs = q_strides
    p.k_bs, p.k_rs = k_strides
    p.v_bs, p.v_rs = v_strides
    p.o_bs, p.o_rs = o_strides
    p.scale = scale
    p.mask = _p(mask)
    if mask is None:
        p.mask_mode = 0
    elif mask.dim() == 2:
        p.mask_mode = 1
    else:
        p.mask_mode = 2
    return p


def attn_fwd(q, k, v, o, lse, *, B, H, Sq, Sk, hd, scale, mask=None, q_strides, k_strides, v_strides, o_strides, drop=None,
             kv_batch_mod=0, kv_index=None):
    """q/k/v/o are 16-bit tensors (possibly views into one fused projection buffer); *_strides = (batch, row) in
    elements.  mask: additive fp32 [B,Sk] or [B,Sq,Sk].  kv_index (inference): int32 [B] device tensor - batch entry b reads the K/V set
    kv_index[b] (k_strides[0] / v_strides[0] apart); the caller guarantees every value names a set the buffers hold (mico_attn_params.kv_index)."""
    p = _attn_params(B, H, Sq, Sk, hd, q, k, v, o, scale, mask, q_strides, k_strides, v_strides, o_strides, drop, kv_batch_mod, kv_index=kv_index)
    rc = _lib.lib().mico_attn_fwd(_p(q), _p(k), _p(v), _p(o), _p(lse), C.byref(p), dt_code(q.dtype), _st())
    check(rc, "mico_attn_fwd")


DECODE_TARGET_WGS = 2048   # one-wave workgroups of mico_attn_decode the key split aims for (256 CUs x 8 waves in flight)
DECODE_QCHUNK = 4          # queries per workgroup (DEC_QC in csrc/decode.hip)


def attn_decode_splits(sets, H, QR, Sk):
    """Key split of mico_attn_decode: enough workgroups to fill the chip when sets x heads cannot (a whole 64-key block at least per split)."""
    items = sets * H * (-(-QR // DECODE_QCHUNK))
    return max(1, min(-(-Sk // 64), -(-DECODE_TARGET_WGS // items)))


def attn_decode(q, k, v, o, *, sets, rows_per_set, q_per_row, H, Sk, hd, scale, q_rs, kv_strides, o_rs, mask=None, mask_strides=(0, 0),
                splits=None, set_row0=None, rows=None):
    """Grouped-query decode attention (mico_attn_decode): `sets` key sets of Sk keys, each read by rows_per_set x q_per_row queries.
    q / o: 16-bit, query (s, r, i) at row (s rows_per_set + r) q_per_row + i (row strides q_rs / o_rs, head h at columns h hd ..);
    k / v: key n of set s at s kv_strides[0] + n kv_strides[1]; mask: fp32 additive, row of query (s, r, i) at
    (s rows_per_set + r) mask_strides[0] + i mask_strides[1].  splits: key split (None: attn_decode_splits).
    set_row0 (mico_attn_decode_ragged): the sets own different numbers of rows - set s owns the query rows [set_row0[s], set_row0[s + 1]),
    set_row0 a DEVICE int32 [sets + 1] tensor (decode_set_row0) the caller vouches for: ascending from 0 to `rows`, no set larger than
    rows_per_set, which is then the LARGEST set's row count (it sizes the launch and the default key split).  q / o / mask rows are
    addressed by the global row."""
    if hd != 64:
        raise MicoHipError(f"attn_decode: head size {hd} is not supported (hd 64 only)")
    if q.dtype not in (torch.float16, torch.bfloat16) or k.dtype != q.dtype or v.dtype != q.dtype or o.dtype != q.dtype:
        raise MicoHipError("attn_decode: q / k / v / o must share one 16-bit dtype")
    if mask is not None and mask.dtype != torch.float32:
        raise MicoHipError("attn_decode: the mask is fp32 additive")
    if set_row0 is not None and (set_row0.dtype != torch.int32 or set_row0.dim() != 1 or set_row0.numel() != sets + 1
                                 or not set_row0.is_contiguous() or set_row0.device != q.device):
        raise MicoHipError("attn_decode: set_row0 is a contiguous int32 [sets + 1] tensor on the queries' device")
    QR = rows_per_set * q_per_row
    splits = attn_decode_splits(sets, H, QR, Sk) if splits is None else int(splits)
    l = _lib.lib()
    nbytes = l.mico_attn_decode_ws_bytes(sets, H, QR, Sk, splits) if QR <= 0x7fffffff else -1
    if nbytes < 0:
        raise MicoHipError(f"attn_decode: bad shape (sets {sets}, H {H}, rows per set <= {rows_per_set}, q_per_row {q_per_row}, Sk {Sk}, "
                           f"splits {splits})")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device) if nbytes else None
    head = (_p(q), q_rs, _p(k), _p(v), kv_strides[0], kv_strides[1], _p(o), o_rs, _p(mask), mask_strides[0], mask_strides[1], sets)
    tail = (q_per_row, H, Sk, hd, scale, splits, _p(ws), nbytes, dt_code(q.dtype), _st())
    if set_row0 is None:
        check(l.mico_attn_decode(*head, rows_per_set, *tail), "mico_attn_decode")
    else:
        check(l.mico_attn_decode_ragged(*head, _p(set_row0), rows, rows_per_set, *tail), "mico_attn_decode_ragged")


def decode_set_row0(rows_per_set):
    """The first-row table of mico_attn_decode_ragged for sets of rows_per_set[s] rows: host int32 [sets + 1], [0, r0, r0 + r1, ...]."""
    rows = [int(r) for r in rows_per_set]
    if not rows or min(rows) < 0:
        raise ValueError(f"rows per set {rows}: a non-empty sequence of non-negative ints")
    return torch.tensor([0] + rows, dtype=torch.int64).cumsum(0).to(torch.int32)


def attn_decode_ragged(q, k, v, o, *, set_row0, rows, max_rows_per_set, q_per_row, H, Sk, hd, scale, q_rs, kv_strides, o_rs, mask=None,
                       mask_strides=(0, 0), splits=None):
    """attn_decode(set_row0=...) under the library entry point's argument names: sets = set_row0.numel() - 1, `rows` query rows in all."""
    attn_decode(q, k, v, o, sets=set_row0.numel() - 1, rows_per_set=max_rows_per_set, q_per_row=q_per_row, H=H, Sk=Sk, hd=hd, scale=scale,
                q_rs=q_rs, kv_strides=kv_strides, o_rs=o_rs, mask=mask, mask_strides=mask_strides, splits=splits, set_row0=set_row0, rows=rows)


def decode_kv_append(src, cache, *, rows, n_new, pos0):
    """cache [rows, max_len, width] (row stride per position) <- src rows r n_new + i at positions pos0 + i (16-bit, src [rows n_new, >= width])."""
    width = cache.shape[-1]
    check(_lib.lib().mico_decode_kv_append(_p(src), src.stride(0), _p(cache), cache.stride(0), cache.stride(1), rows, n_new, pos0, width, _st()),
          "mico_decode_kv_append")


def decode_kv_gather(src, dst, parent, n):
    """dst[l, r, :n positions] = src[l, parent[r], :n positions] for caches [layers, rows, max_len, width]; parent int64 [rows] on the device."""
    Lr, rows = src.shape[0], src.shape[1]
    assert src.shape == dst.shape and src.is_contiguous() and dst.is_contiguous() and parent.dtype == torch.int64 and parent.numel() == rows
    check(_lib.lib().mico_decode_kv_gather(_p(src), _p(dst), _p(parent.contiguous()), Lr, rows, src.stride(0), src.stride(1),
                                           n * src.stride(2), _st()), "mico_decode_kv_gather")


def attn_bwd(q, k, v, o, do, lse, dq, dk, dv, delta, *, B, H, Sq, Sk, hd, scale, mask=None, q_strides, k_strides,
             v_strides, o_strides, drop=None, kv_batch_mod=0, batch0=0, dkv_accumulate=False, kv_index=None):
    """kv_batch_mod > 0: k / v hold kv_batch_mod batch entries shared modulo (see mico_attn_params); dk / dv are [B, ...] as always.
    batch0: this launch covers entries batch0 .. batch0 + B of a larger batch (dropout counters); dkv_accumulate: dk / dv += (short-query kernel)."""
    p = _attn_params(B, H, Sq, Sk, hd, q, k, v, o, scale, mask, q_strides, k_strides, v_strides, o_strides, drop, kv_batch_mod, batch0, dkv_accumulate,
                     kv_index=kv_index)      # (kv_index: refused by the library - the forward's inference-only indexed K/V has no backward)
    rc = _lib.lib().mico_attn_bwd(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(dq), _p(dk), _p(dv), _p(delta),
                                  C.byref(p), dt_code(q.dtype), _st())
    check(rc, "mico_attn_bwd")


def rope(x, bs, rs, B, N, H, hd, cos_t, sin_t, inverse=False):
    check(_lib.lib().mico_rope(_p(x), bs, rs, B, N, H, hd, _p(cos_t), _p(sin_t), int(inverse), dt_code(x.dtype), _st()),
          "mico_rope")


def im2row(pixels, rows16, P, kpad):
    B, Cc, H, W = pixels.shape
    check(_lib.lib().mico_im2row(_p(pixels), _p(rows16), B, Cc, H, W, P, kpad, dt_code(rows16.dtype), _st()), "mico_im2row")


def _keep_i32(keep):
    if keep.dtype != torch.int32 or not keep.is_contiguous() or keep.dim() != 2:
        raise MicoHipError("patch-dropout keep tables are contiguous int32 [frames, keep] device tensors")
    return keep


def im2row_keep(pixels, rows16, keep, P, kpad):
    """rows16 [B * keep, kpad] = im2row of the kept patches (keep: int32 [B, keep])."""
    B, Cc, H, W = pixels.shape
    keep = _keep_i32(keep)
    assert keep.shape[0] == B and rows16.shape[0] >= B * keep.shape[1]
    check(_lib.lib().mico_im2row_keep(_p(pixels), _p(rows16), _p(keep), B, Cc, H, W, P, kpad, keep.shape[1], dt_code(rows16.dtype), _st()),
          "mico_im2row_keep")


def patch_pos_keep(x, keep, cls, pos):
    """x fp32 [B * (1 + keep), D] after the bias-only patch GEMM: CLS rows = cls + pos[0], kept rows += pos[1 + keep[f, r]]."""
    keep = _keep_i32(keep)
    B, nk = keep.shape
    np_ = pos.shape[0] - 1
    assert x.shape[0] >= B * (nk + 1) and pos.shape[1] == x.shape[1] == cls.numel() and pos.is_contiguous()
    check(_lib.lib().mico_patch_pos_keep(_p(x), x.stride(0), _p(keep), B, nk, _p(cls), _p(pos), np_, x.shape[1], _st()), "mico_patch_pos_keep")


def rope_keep(x, bs, rs, B, N, H, hd, cos_t, sin_t, keep, frame_map=None, inverse=False):
    """ops.rope with per-frame table rows: token 1 + n of frame b uses row keep[frame_map[b] if frame_map is not None else b, n]."""
    keep = _keep_i32(keep)
    assert keep.shape[1] == N - 1
    check(_lib.lib().mico_rope_keep(_p(x), bs, rs, B, N, H, hd, _p(cos_t), _p(sin_t), _p(keep), keep.shape[0], _p(frame_map),
                                    cos_t.shape[0], int(inverse), dt_code(x.dtype), _st()), "mico_rope_keep")


def pos_grad_keep(g, keep, np_, dpos=None, inv_ws=None):
    """Positional-table gradient of a dropped pass: g fp32 [B * (1 + keep), D] -> dpos fp32 [1 + np_, D] (deterministic, no atomics)."""
    keep = _keep_i32(keep)
    B, nk = keep.shape
    D = g.shape[1]
    assert g.shape[0] >= B * (nk + 1)
    dpos = dpos if dpos is not None else torch.empty((np_ + 1, D), dtype=torch.float32, device=g.device)
    inv_ws = inv_ws if inv_ws is not None else torch.empty(max(1, B * np_), dtype=torch.int32, device=g.device)
    assert dpos.is_contiguous() and dpos.numel() >= (np_ + 1) * D and inv_ws.numel() >= B * np_
    check(_lib.lib().mico_pos_grad_keep(_p(g), g.stride(0), _p(keep), B, nk, np_, D, _p(inv_ws), _p(dpos), _st()), "mico_pos_grad_keep")
    return dpos


def cast_f32_to_16(src, dst, *, cols=None, cols_pad=None, scale=1.0):
    rows = src.shape[0]
    cols = cols if cols is not None else src.shape[1]
    cols_pad = cols_pad if cols_pad is not None else dst.shape[1]
    check(_lib.lib().mico_cast_f32_to_16(_p(src), src.stride(0), _p(dst), dst.stride(0), rows, cols, cols_pad, scale,
                                         dt_code(dst.dtype), _st()), "mico_cast_f32_to_16")
    return dst


def cast_16_to_f32(src, dst, *, scale=1.0, accumulate=False):
    rows, cols = src.shape
    check(_lib.lib().mico_cast_16_to_f32(_p(src), src.stride(0), _p(dst), dst.stride(0), rows, cols, scale,
                                         int(accumulate), dt_code(src.dtype), _st()), "mico_cast_16_to_f32")
    return dst


def gather_rows_cast(src, dst, *, remap=(0, 0, 0), row_scale=None, rows_per_scale=0, scale=1.0, frame_map=None,
                     rows_per_frame=0, dst_map=None):
    """dst_map: the frames listed in frame_map land in the frame slots dst_map[j] of dst (only those rows are written)."""
    rows, cols = dst.shape
    if dst_map is not None:
        rows = frame_map.numel() * rows_per_frame
    check(_lib.lib().mico_gather_rows_cast(_p(src), src.stride(0), _p(dst), dst.stride(0), rows, cols, remap[0], remap[1],
                                           remap[2], _p(row_scale), rows_per_scale, scale, _p(frame_map), rows_per_frame,
                                           _p(dst_map), dt_code(dst.dtype), _st()),
          "mico_gather_rows_cast")
    return dst


def colsum(x, out, *, rows=None, cols=None, ld=None, scale=1.0, accumulate=False):
    rows = rows if rows is not None else x.shape[0]
    cols = cols if cols is not None else x.shape[1]
    ld = ld if ld is not None else x.stride(0)
    check(_lib.lib().mico_colsum(_p(x), dt_code(x.dtype), ld, rows, cols, _p(out), scale, int(accumulate), _st()),
          "mico_colsum")
    return out


def dw_colfold(dwt, dbt, gamma, beta, dw, db=None):
    """dw[m, n] += dwt[m, n] * gamma[n] + dbt[m] * beta[n];  db[m] += dbt[m]  (mico_dw_colfold: a LayerNorm's affine folded into the weight
    gradient of the Linear it feeds - dwt / dbt come from the weight-gradient GEMM against the normalised rows)."""
    M, N = dwt.shape
    assert dwt.is_contiguous() and dwt.dtype == dbt.dtype == gamma.dtype == beta.dtype == dw.dtype == torch.float32 and dw.stride(1) == 1
    assert dw.shape[0] >= M and dw.shape[1] == N and dbt.numel() >= M and gamma.numel() == N and beta.numel() == N
    check(_lib.lib().mico_dw_colfold(_p(dwt), _p(dbt), _p(gamma), _p(beta), _p(dw), dw.stride(0), _p(db), M, N, _st()), "mico_dw_colfold")


def cls_rows(x, B, group_rows, cls, pos0):
    check(_lib.lib().mico_cls_rows(_p(x), x.stride(0), B, group_rows, _p(cls), _p(pos0), x.shape[1], _st()), "mico_cls_rows")


def add_f32(a, b, y=None, y16=None, scale16=1.0, dtype=torch.float16):
    check(_lib.lib().mico_add_f32(_p(a), _p(b), _p(y), _p(y16), a.numel(), scale16,
                                  dt_code(y16.dtype if y16 is not None else dtype), _st()), "mico_add_f32")


def swiglu_fwd(x1, x2, h):
    check(_lib.lib().mico_swiglu_fwd(_p(x1), _p(x2), _p(h), x1.numel(), dt_code(x1.dtype), _st()), "mico_swiglu_fwd")


def swiglu_fwd_f32(x1, x2, h):
    check(_lib.lib().mico_swiglu_fwd_f32(_p(x1), _p(x2), _p(h), x1.numel(), _st()), "mico_swiglu_fwd_f32")


def swiglu_bwd(x1, x2, dh, dx1, dx2):
    check(_lib.lib().mico_swiglu_bwd(_p(x1), _p(x2), _p(dh), _p(dx1), _p(dx2), x1.numel(), dt_code(x1.dtype), _st()),
          "mico_swiglu_bwd")


def bert_embed_fwd(ids, word, pos, type0, out, S):
    rows, cols = out.shape
    check(_lib.lib().mico_bert_embed_fwd(_p(ids), _p(word), _p(pos), _p(type0), _p(out), rows, S, cols, word.shape[0], _st()),
          "mico_bert_embed_fwd")


def embed_scatter_add(ids, dsum, dword, dpos, dtype0, S, scale=1.0):
    rows, cols = dsum.shape
    vocab = dword.shape[0] if dword is not None else 0
    check(_lib.lib().mico_embed_scatter_add(_p(ids), _p(dsum), _p(dword), _p(dpos), _p(dtype0), rows, S, cols, vocab, scale,
                                            _st()), "mico_embed_scatter_add")


def ce_fwd_bwd(logits, target, *, cols=None, ignore_index=-100, label_smoothing=0.0, logits_scale=1.0, row_loss=None,
               row_lse=None, dlogits=None, dscale_ptr=None, dscale=1.0):
    rows = logits.shape[0]
    cols = cols if cols is not None else logits.shape[1]
    check(_lib.lib().mico_ce_fwd_bwd(_p(logits), dt_code(logits.dtype), logits.stride(0), rows, cols, _p(target),
                                     ignore_index, label_smoothing, logits_scale, _p(row_loss), _p(row_lse), _p(dlogits),
                                     dt_code(dlogits.dtype) if dlogits is not None else 0,
                                     dlogits.stride(0) if dlogits is not None else 0, _p(dscale_ptr), dscale, 0, _st()),
          "mico_ce_fwd_bwd")


def logprob_fwd_bwd(logits, target, *, cols=None, ignore_index=-100, row_logp=None, dlogits=None, row_gscale=None, gscale=1.0):
    """Per-row log P(target) and / or its gradient with one upstream gradient per row; see mico_logprob_fwd_bwd."""
    rows = logits.shape[0]
    cols = cols if cols is not None else logits.shape[1]
    if dlogits is not None and (dlogits.dtype != logits.dtype or row_gscale is None or row_gscale.dtype != torch.float32
                                or row_gscale.numel() != rows or not row_gscale.is_contiguous()):
        raise MicoHipError("logprob_fwd_bwd: dlogits has the logits' dtype and needs row_gscale, contiguous fp32 [rows]")
    check(_lib.lib().mico_logprob_fwd_bwd(_p(logits), dt_code(logits.dtype), logits.stride(0), rows, cols, _p(target), ignore_index,
                                          _p(row_logp), _p(dlogits), dlogits.stride(0) if dlogits is not None else 0, _p(row_gscale),
                                          float(gscale), _st()), "mico_logprob_fwd_bwd")


def vocab_sample(logits, u, *, cols=None, unfinished=None, eos_token_id=None, pad_token_id=0):
    """(token int64 [rows], logp fp32 [rows]): one inverse-CDF draw per row of the fp32 logits [rows, >= cols] (any row stride) from
    softmax(logits[:, :cols]) with the uniform numbers u fp32 [rows]; see mico_vocab_sample.  unfinished: bool / uint8 [rows], updated in
    place - finished rows emit pad_token_id with logp 0, a row that draws eos_token_id becomes finished."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise MicoHipError(f"vocab_sample takes a 2-D fp32 matrix with unit column stride (got {logits.dtype} {tuple(logits.shape)})")
    rows = logits.shape[0]
    cols = int(cols) if cols is not None else logits.shape[1]
    if not 0 < cols <= logits.shape[1]:
        raise MicoHipError(f"vocab_sample: cols = {cols} of a row of {logits.shape[1]}")
    if u.dtype != torch.float32 or u.numel() != rows:
        raise MicoHipError("vocab_sample: u is fp32 [rows]")
    if unfinished is not None and (unfinished.dtype not in (torch.bool, torch.uint8) or unfinished.numel() != rows
                                   or not unfinished.is_contiguous()):
        raise MicoHipError("vocab_sample: unfinished is a contiguous bool / uint8 [rows] tensor")
    token = torch.empty(rows, dtype=torch.int64, device=logits.device)
    logp = torch.empty(rows, dtype=torch.float32, device=logits.device)
    if rows == 0:
        return token, logp
    check(_lib.lib().mico_vocab_sample(_p(logits), logits.stride(0) if rows > 1 else max(logits.stride(0), cols), rows, cols,
                                       _p(u.contiguous()), _p(unfinished), -1 if eos_token_id is None else int(eos_token_id),
                                       int(pad_token_id or 0), _p(token), _p(logp), _st()), "mico_vocab_sample")
    return token, logp


BEAM_NB_MAX = 8   # largest num_beams of the device-side beam search (BEAM_NB_MAX in csrc/beam.hip)


def beam_topk(logits, beam_scores, num_beams, *, cols=None, done=None, ids=None, cur_len=None, repetition_penalty=1.0,
              no_repeat_ngram_size=0, ban_eos=False, eos_token_id=None, out=None):
    """(score fp32, beam int32, token int32), each [sets, 2 num_beams]: per set of num_beams consecutive rows of the fp32 logits [rows, >= cols]
    (any row stride) the 2 num_beams best of log_softmax(logits[row, :cols]) (processed) + beam_scores[row], descending, equal scores by
    ascending beam * cols + token; see mico_beam_topk.  done: bool / uint8 [sets], a done set's outputs are left untouched (`out`: the three
    tensors to write into).  ids int64 [rows, >= cur_len] (any row stride) switches the processors on: repetition_penalty,
    no_repeat_ngram_size, ban_eos (eos_token_id at -inf)."""
    nb = int(num_beams)
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise MicoHipError(f"beam_topk takes a 2-D fp32 matrix with unit column stride (got {logits.dtype} {tuple(logits.shape)})")
    rows = logits.shape[0]
    cols = int(cols) if cols is not None else logits.shape[1]
    if not 0 < cols <= logits.shape[1]:
        raise MicoHipError(f"beam_topk: cols = {cols} of a row of {logits.shape[1]}")
    if nb < 1 or rows % nb:
        raise MicoHipError(f"beam_topk: {rows} rows are not a whole number of sets of {nb} beams")
    sets = rows // nb
    if beam_scores.dtype != torch.float32 or beam_scores.numel() != rows or not beam_scores.is_contiguous():
        raise MicoHipError("beam_topk: beam_scores is a contiguous fp32 [rows] tensor")
    if done is not None and (done.dtype not in (torch.bool, torch.uint8) or done.numel() != sets or not done.is_contiguous()):
        raise MicoHipError("beam_topk: done is a contiguous bool / uint8 [sets] tensor")
    ld_ids = 0
    if ids is not None:
        cur_len = ids.shape[1] if cur_len is None else int(cur_len)
        if ids.dim() != 2 or ids.dtype != torch.int64 or ids.shape[0] != rows or (ids.shape[1] and ids.stride(1) != 1) or cur_len > ids.shape[1]:
            raise MicoHipError(f"beam_topk: ids is int64 [rows, >= cur_len] with unit column stride (got {ids.dtype} {tuple(ids.shape)})")
        ld_ids = ids.stride(0) if rows > 1 else max(ids.stride(0), cur_len)
    K = 2 * nb
    dev = logits.device
    if out is None:
        out = (torch.empty(sets, K, dtype=torch.float32, device=dev), torch.empty(sets, K, dtype=torch.int32, device=dev),
               torch.empty(sets, K, dtype=torch.int32, device=dev))
    score, beam, token = out
    for t, dt in ((score, torch.float32), (beam, torch.int32), (token, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (sets, K) or not t.is_contiguous():
            raise MicoHipError("beam_topk: out is (fp32, int32, int32) contiguous [sets, 2 num_beams] tensors")
    if rows == 0:
        return score, beam, token
    ws = torch.empty(rows * K, dtype=torch.int64, device=dev)
    check(_lib.lib().mico_beam_topk(_p(logits), logits.stride(0) if rows > 1 else max(logits.stride(0), cols), sets, nb, cols, _p(beam_scores),
                                    _p(done), _p(ids), ld_ids, int(cur_len or 0), float(repetition_penalty), int(no_repeat_ngram_size),
                                    int(bool(ban_eos)), -1 if eos_token_id is None else int(eos_token_id), _p(ws), _p(score), _p(beam), _p(token),
                                    _st()), "mico_beam_topk")
    return score, beam, token


class BeamState:
    """The device-side state of one beam search (mico_beam_step / mico_beam_finalize): per set of num_beams rows the n-best list of finished
    hypotheses (ids, lengths, fp64 scores in insertion order, count, worst score), the sticky `done` byte, and the counter of sets not yet
    done.  len_pow: len ** length_penalty for len = 0 .. max_length, computed here by Python and uploaded once, so the device divides by the
    very numbers the host search divides by."""

    def __init__(self, sets, num_beams, max_length, length_penalty, device):
        self.sets, self.nb, self.max_length = int(sets), int(num_beams), int(max_length)
        if not 1 <= self.nb <= BEAM_NB_MAX:
            raise MicoHipError(f"BeamState: num_beams = {num_beams} (1 .. {BEAM_NB_MAX})")
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self.len_pow = torch.tensor([float(n ** length_penalty) for n in range(self.max_length + 1)], dtype=torch.float64).to(device)
        self.hyp_ids = z((self.sets, self.nb, self.max_length), torch.int64)
        self.hyp_len, self.hyp_score = z((self.sets, self.nb), torch.int32), z((self.sets, self.nb), torch.float64)
        self.hyp_count = z((self.sets,), torch.int32)
        self.worst = torch.full((self.sets,), 1e9, dtype=torch.float64, device=device)
        self.done = z((self.sets,), torch.uint8)
        self.not_done = torch.full((1,), self.sets, dtype=torch.int32, device=device)

    def params(self, cur_len, eos_token_id, pad_token_id, ids_in, beam_scores):
        rows = self.sets * self.nb
        if ids_in.dtype != torch.int64 or tuple(ids_in.shape) != (rows, self.max_length) or not ids_in.is_contiguous():
            raise MicoHipError(f"beam search: ids buffers are contiguous int64 [{rows}, {self.max_length}] (got {ids_in.dtype} {tuple(ids_in.shape)})")
        if beam_scores.dtype != torch.float32 or beam_scores.numel() != rows or not beam_scores.is_contiguous():
            raise MicoHipError("beam search: beam_scores is a contiguous fp32 [rows] tensor")
        p = _lib.BeamParams()
        p.sets, p.nb, p.cur_len, p.max_length = self.sets, self.nb, int(cur_len), self.max_length
        p.eos_id, p.pad_id = -1 if eos_token_id is None else int(eos_token_id), int(pad_token_id or 0)
        p.len_pow, p.ids_in, p.beam_scores = _p(self.len_pow), _p(ids_in), _p(beam_scores)
        p.hyp_ids, p.hyp_len, p.hyp_score, p.hyp_count = _p(self.hyp_ids), _p(self.hyp_len), _p(self.hyp_score), _p(self.hyp_count)
        p.worst, p.done, p.not_done = _p(self.worst), _p(self.done), _p(self.not_done)
        return p


def beam_step(state, cand, ids_in, ids_out, cur_len, beam_scores, parent, *, eos_token_id=None, pad_token_id=0):
    """One step of the search bookkeeping on the device; see mico_beam_step.  cand: beam_topk's (score, beam, token); ids_in / ids_out: the two
    halves of the int64 [rows, max_length] double buffer, rows of ids_in cur_len long; beam_scores fp32 [rows] and parent int64 [rows] are
    written (the next step's scores; ids_out[r, :cur_len] = ids_in[parent[r], :cur_len], ids_out[r, cur_len] = the row's new token)."""
    rows, K = state.sets * state.nb, 2 * state.nb
    score, beam, token = cand
    for t, dt in ((score, torch.float32), (beam, torch.int32), (token, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (state.sets, K) or not t.is_contiguous():
            raise MicoHipError("beam_step: cand is beam_topk's (fp32, int32, int32) [sets, 2 num_beams] tensors")
    if parent.dtype != torch.int64 or parent.numel() != rows or not parent.is_contiguous():
        raise MicoHipError("beam_step: parent is a contiguous int64 [rows] tensor")
    if tuple(ids_out.shape) != tuple(ids_in.shape) or ids_out.dtype != torch.int64 or not ids_out.is_contiguous() or ids_out.data_ptr() == ids_in.data_ptr():
        raise MicoHipError("beam_step: ids_out is the other half of the ids double buffer")
    p = state.params(cur_len, eos_token_id, pad_token_id, ids_in, beam_scores)
    p.cand_score, p.cand_beam, p.cand_token, p.ids_out, p.parent = _p(score), _p(beam), _p(token), _p(ids_out), _p(parent)
    check(_lib.lib().mico_beam_step(C.byref(p), _st()), "mico_beam_step")


def beam_finalize(state, ids_in, cur_len, beam_scores, *, eos_token_id=None, pad_token_id=0):
    """(best ids int64 [sets, max_length], lengths int32 [sets]): sets not done add their open beams (rows of ids_in, cur_len long, with
    beam_scores), then every set's best hypothesis, eos-terminated and pad-filled; see mico_beam_finalize."""
    p = state.params(cur_len, eos_token_id, pad_token_id, ids_in, beam_scores)
    best = torch.empty(state.sets, state.max_length, dtype=torch.int64, device=ids_in.device)
    lens = torch.empty(state.sets, dtype=torch.int32, device=ids_in.device)
    p.best_ids, p.best_len = _p(best), _p(lens)
    check(_lib.lib().mico_beam_finalize(C.byref(p), _st()), "mico_beam_finalize")
    return best, lens


SAMPLE_TOPK_MAX = 64   # largest top_k of mico_warp_sample (SAMPLE_K_MAX in csrc/sample.hip)


def warp_sample(logits, u, *, cols=None, ids=None, cur_len=None, top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0,
                no_repeat_ngram_size=0, ban_eos=False, eos_token_id=None, pad_token_id=0, unfinished=None, not_done=None, append=False,
                out=None):
    """(token int64, logp fp32, n_kept int32, kept_min fp32), each [rows]: one sampling decode step per row of the fp32 logits [rows, >= cols]
    (any row stride) with the uniform numbers u fp32 [rows] - logits processors, temperature, top-k (0: off, <= SAMPLE_TOPK_MAX), top-p, one
    inverse-CDF draw; see mico_warp_sample.  ids int64 [rows, >= cur_len] (any row stride) switches the processors on (repetition_penalty,
    no_repeat_ngram_size, ban_eos) and, with append, receives the token in column cur_len.  unfinished: bool / uint8 [rows], updated in place
    (finished rows emit pad_token_id; a row that draws eos_token_id becomes finished and decrements not_done, int32 [1]).  out: the four
    tensors to write into.  The kernel's limits are its own: a refused call raises MicoHipError before anything is launched."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise MicoHipError(f"warp_sample takes a 2-D fp32 matrix with unit column stride (got {logits.dtype} {tuple(logits.shape)})")
    rows = logits.shape[0]
    cols = int(cols) if cols is not None else logits.shape[1]
    if cols > logits.shape[1]:
        raise MicoHipError(f"warp_sample: cols = {cols} of a row of {logits.shape[1]}")
    if u.dtype != torch.float32 or u.numel() != rows:
        raise MicoHipError("warp_sample: u is fp32 [rows]")
    if unfinished is not None and (unfinished.dtype not in (torch.bool, torch.uint8) or unfinished.numel() != rows
                                   or not unfinished.is_contiguous()):
        raise MicoHipError("warp_sample: unfinished is a contiguous bool / uint8 [rows] tensor")
    if not_done is not None and (not_done.dtype != torch.int32 or not_done.numel() != 1):
        raise MicoHipError("warp_sample: not_done is an int32 [1] tensor")
    ld_ids = 0
    if ids is not None:
        cur_len = ids.shape[1] if cur_len is None else int(cur_len)
        if ids.dim() != 2 or ids.dtype != torch.int64 or ids.shape[0] != rows or (ids.shape[1] and ids.stride(1) != 1) or cur_len > ids.shape[1]:
            raise MicoHipError(f"warp_sample: ids is int64 [rows, >= cur_len] with unit column stride (got {ids.dtype} {tuple(ids.shape)})")
        ld_ids = ids.stride(0) if rows > 1 else ids.shape[1]
        if append and ld_ids > ids.shape[1] <= cur_len:      # (a narrowed view: the kernel's own check sees the stride only)
            raise MicoHipError(f"warp_sample: append writes column cur_len = {cur_len} of ids {tuple(ids.shape)}")
    dev = logits.device
    if out is None:
        out = (torch.empty(rows, dtype=torch.int64, device=dev), torch.empty(rows, dtype=torch.float32, device=dev),
               torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev))
    token, logp, n_kept, kept_min = out
    for t, dt in ((token, torch.int64), (logp, torch.float32), (n_kept, torch.int32), (kept_min, torch.float32)):
        if t.dtype != dt or t.numel() != rows or not t.is_contiguous():
            raise MicoHipError("warp_sample: out is (int64, fp32, int32, fp32) contiguous [rows] tensors")
    if rows == 0:
        return token, logp, n_kept, kept_min
    p = _lib.WarpSampleParams()
    p.logits, p.ld, p.rows, p.V = _p(logits), logits.stride(0) if rows > 1 else max(logits.stride(0), cols), rows, cols
    p.u, p.ids, p.ld_ids, p.cur_len = _p(u.contiguous()), _p(ids), ld_ids, int(cur_len or 0)
    p.top_k, p.top_p, p.temperature = int(top_k), float(top_p), float(temperature)
    p.rep_penalty, p.ngram, p.ban_eos = float(repetition_penalty), int(no_repeat_ngram_size), int(bool(ban_eos))
    p.eos_id, p.pad_id = -1 if eos_token_id is None else int(eos_token_id), int(pad_token_id or 0)
    p.unfinished, p.not_done, p.append = _p(unfinished), _p(not_done), int(bool(append))
    p.token, p.logp, p.n_kept, p.kept_min = _p(token), _p(logp), _p(n_kept), _p(kept_min)
    check(_lib.lib().mico_warp_sample(C.byref(p), _st()), "mico_warp_sample")
    return token, logp, n_kept, kept_min


def token_mask(tokens, mask_prob, u_mask, u_kind, u_tok, mask_token, range_start, range_end):
    """(masked token ids, labels) of the caption loss's TokenMasker on the device; see mico_token_mask.  u_mask [rounds, rows, S]."""
    rows, S = tokens.shape
    toks = tokens.contiguous()
    out, labels = torch.empty_like(toks), torch.empty_like(toks)
    check(_lib.lib().mico_token_mask(_p(toks), rows, S, float(mask_prob), _p(u_mask.contiguous()), u_mask.shape[0], _p(u_kind.contiguous()),
                                     _p(u_tok.contiguous()), int(mask_token), int(range_start), int(range_end), _p(out), _p(labels), _st()),
          "mico_token_mask")
    return out, labels


def itm_sample(sim, diag_offset, u):
    """One hard-negative index per row of the fp32 similarity logits `sim` [rows, cols]; see mico_itm_sample."""
    sim = sim.contiguous()
    out = torch.empty(sim.shape[0], dtype=torch.int64, device=sim.device)
    check(_lib.lib().mico_itm_sample(_p(sim), sim.stride(0), sim.shape[0], sim.shape[1], int(diag_offset), _p(u.contiguous()), _p(out), _st()),
          "mico_itm_sample")
    return out


TOPK_MAX = 128   # largest k of mico_topk_rows (TOPK_MAX in csrc/loss.hip)


def topk_rows(sim, k):
    """(values fp32 [rows, k], indices int32 [rows, k]) - the k largest entries of every row of the fp32 matrix `sim` in descending order, equal
    values by ascending column (mico_topk_rows: one pass over the matrix, no sort workspace).  1 <= k <= min(TOPK_MAX, cols)."""
    if sim.dim() != 2 or sim.dtype != torch.float32:
        raise MicoHipError(f"topk_rows takes a 2-D fp32 matrix (got {sim.dtype} {tuple(sim.shape)})")
    if sim.stride(1) != 1:
        sim = sim.contiguous()
    rows, cols = sim.shape
    idx = torch.empty((rows, int(k)), dtype=torch.int32, device=sim.device)
    val = torch.empty((rows, int(k)), dtype=torch.float32, device=sim.device)
    if rows == 0:
        if not sim.is_cuda:
            _p(sim)
        return val, idx
    check(_lib.lib().mico_topk_rows(_p(sim), sim.stride(0) if rows > 1 else cols, rows, cols, int(k), _p(idx), _p(val), _st()), "mico_topk_rows")
    return val, idx


def win_attn_fwd(qkv, out, lse, bias_table, batch, res, heads, shift, scale):
    """Swin (shifted-)window attention in token order; see mico_win_attn_fwd."""
    check(_lib.lib().mico_win_attn_fwd(_p(qkv), _p(out), _p(lse), _p(bias_table), batch, res, heads, shift, float(scale), dt_code(qkv.dtype),
                                       _st()), "mico_win_attn_fwd")


def win_attn_bwd(qkv, dout, lse, bias_table, dqkv, dbias_table, batch, res, heads, shift, scale, dbias_scale=1.0):
    check(_lib.lib().mico_win_attn_bwd(_p(qkv), _p(dout), _p(lse), _p(bias_table), _p(dqkv), _p(dbias_table), batch, res, heads, shift,
                                       float(scale), float(dbias_scale), dt_code(qkv.dtype), _st()), "mico_win_attn_bwd")


def patch_merge(x, out, batch, res, channels, backward=False):
    """PatchMerging's 2x2 gather on the fp32 stream ([batch, res*res, C] -> [batch, res*res/4, 4C]) or its inverse (backward)."""
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and x.is_contiguous() and out.is_contiguous()
    check(_lib.lib().mico_patch_merge(_p(x), _p(out), batch, res, channels, int(bool(backward)), _st()), "mico_patch_merge")


def l2norm_fwd(x, y, inv_norm):
    check(_lib.lib().mico_l2norm_fwd(_p(x), _p(y), _p(inv_norm), x.shape[0], x.shape[1], _st()), "mico_l2norm_fwd")


def l2norm_bwd(dy, y, inv_norm, dx):
    check(_lib.lib().mico_l2norm_bwd(_p(dy), _p(y), _p(inv_norm), _p(dx), y.shape[0], y.shape[1], _st()), "mico_l2norm_bwd")


def sgemm(A, B, out, *, ta=False, tb=False, M=None, N=None, K=None, alpha=1.0, beta=0.0, bias=None):
    """Exact fp32 small GEMM (heads / similarity matrices)."""
    if M is None:
        M = A.shape[1] if ta else A.shape[0]
    if K is None:
        K = A.shape[0] if ta else A.shape[1]
    if N is None:
        N = B.shape[1] if tb else B.shape[0]
    check(_lib.lib().mico_sgemm_small(int(ta), int(tb), M, N, K, _p(A), A.stride(0), _p(B), B.stride(0), _p(out),
                                      out.stride(0), alpha, beta, _p(bias), _st()), "mico_sgemm_small")
    return out


def gelu_f32(x, y):
    check(_lib.lib().mico_gelu_f32(_p(x), _p(y), x.numel(), _st()), "mico_gelu_f32")


def gelu_bwd_f32(x, dy, dx):
    check(_lib.lib().mico_gelu_bwd_f32(_p(x), _p(dy), _p(dx), x.numel(), _st()), "mico_gelu_bwd_f32")


def gelu_16(x, y):
    check(_lib.lib().mico_gelu_16(_p(x), _p(y), x.numel(), dt_code(x.dtype), _st()), "mico_gelu_16")


def gelu_bwd_16(x, dy, dx):
    check(_lib.lib().mico_gelu_bwd_16(_p(x), _p(dy), _p(dx), x.numel(), dt_code(x.dtype), _st()), "mico_gelu_bwd_16")


def cls_pool_fwd(tokens, pooled, b, n, frame_stride, D):
    check(_lib.lib().mico_cls_pool_fwd(_p(tokens), _p(pooled), b, n, frame_stride, D, _st()), "mico_cls_pool_fwd")


def cls_pool_bwd(dpooled, dtokens, b, n, frame_stride, D):
    check(_lib.lib().mico_cls_pool_bwd(_p(dpooled), _p(dtokens), b, n, frame_stride, D, _st()), "mico_cls_pool_bwd")


def pool_video_fwd(tokens, pooled, frames, N, D):
    check(_lib.lib().mico_pool_video_fwd(_p(tokens), _p(pooled), frames, N, D, _st()), "mico_pool_video_fwd")


def pool_video_bwd(dpooled, dtokens, frames, N, D):
    check(_lib.lib().mico_pool_video_bwd(_p(dpooled), _p(dtokens), frames, N, D, _st()), "mico_pool_video_bwd")
