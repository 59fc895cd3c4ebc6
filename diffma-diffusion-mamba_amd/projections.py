"""The dense products of the projections (in_proj, out_proj, x_proj, dt_proj): which kernel runs one (`route`), how it is issued
(`product`), and the mixers' linear layers on top (`linear_splitk`, `linear_pair`).  Per projection y = x W^T:
    FWD x [M, K], W [N, K] -> [M, N]        DGRAD dy [M, N], W [N, K] -> [M, K]        WGRAD dy [M, N], x [M, K] -> [N, K] in fp32
hip_ops.gemm_supported / gemm_large_supported say what the kernels CAN take; `route` says what they SHOULD take.  The library calls
keep the exact form (ATen entry, operand shapes and strides) each caller class has always issued: tuned/gemm_gfx950.csv is keyed by it.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import hip_ops
from .step_prep import cast_weight, stacked_pair


class GemmChain:
    """Used only by the opt-in two-stream mode of the block (mamba_block.Spiral_MambaBlock._mixers): every GEMM of the two
    mixer streams is chained behind the previous one with an event, so that no two library GEMMs are ever resident together.
    hipBLASLt / Tensile's persistent stream-K kernels spin-wait for their own not-yet-scheduled workgroups; two of them
    co-scheduled from two queues can starve each other (observed as a GPU hang).  GEMM next to scan / conv / merge kernels
    stays concurrent -- those workgroups always retire."""
    enabled = False
    event = None
    stream = None

    @classmethod
    def run(cls, fn, *args, **kw):
        if not cls.enabled or not torch.cuda.is_available():
            return fn(*args, **kw)
        cur = torch.cuda.current_stream()
        if cls.event is not None and cls.stream != cur:
            cur.wait_event(cls.event)
        out = fn(*args, **kw)
        cls.event = torch.cuda.Event()
        cls.event.record(cur)
        cls.stream = cur
        return out


def _tn_splitk(a, b):
    return GemmChain.run(_tn_splitk_impl, a, b)


_MM_F32 = [None]          # does torch.mm take out_dtype on this device?  (aten::mm.dtype: 16-bit operands, fp32 result, one launch)


def _mm_f32(x, y):
    """x @ y in fp32 from 16-bit operands WITHOUT a separate cast launch where the library offers it (hipBLASLt accumulates in fp32
    anyway; the 16-bit result + `.float()` of the plain form rounds the weight gradient once more and costs a launch per GEMM -- ~150 per
    training step, which is what a small-batch step is made of)."""
    if x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and _MM_F32[0] is not False:
        try:
            out = torch.mm(x, y, out_dtype=torch.float32)
            _MM_F32[0] = True
            return out
        except (RuntimeError, NotImplementedError, TypeError):
            if _MM_F32[0]:                       # it worked before: a real error, not a missing feature
                raise
            _MM_F32[0] = False
    return (x @ y).float()


def _tn_splitk_impl(a, b):
    """a^T @ b for tall operands a (M, P), b (M, Q): the reduction runs over M = B*L or ndir*B*L (50 176 /
    150 528 at the bench shape), which hipBLASLt does not split -- a single-pass GEMM is 2-8x off its memory
    time (x_proj: 492 us vs 82 us; in_proj: 194 us vs 128 us even after solution tuning; tools/bench_gemm.py).
    Split K into C slabs with one bmm and add the slabs in fp32; C is bounded so that the slab outputs stay
    small next to the operands."""
    M = a.shape[0]

    def slabs(t, C):
        """[M, P] (row stride >= P: a column block of a wider row-major buffer is fine, bmm takes the leading dimension) -> [C, M/C, P]"""
        return t.as_strided((C, M // C, t.shape[1]), (M // C * t.stride(0), t.stride(0), 1))

    for C in (64, 32, 16, 8):
        # (below ~12k rows one GEMM is as fast as the slab product + its sum, and it is one launch instead of two: the small-batch step
        #  is made of launches)
        if M >= 12288 and M % C == 0 and M // C >= 256 and C * a.shape[1] * b.shape[1] <= (1 << 23) and a.stride(1) == 1 and b.stride(1) == 1:
            return torch.bmm(slabs(a, C).transpose(1, 2), slabs(b, C)).sum(0, dtype=torch.float32)      # the cast is fused into the reduction
    return _mm_f32(a.t(), b)


# Small launches run on dm_gemm (csrc/gemm.hip); for the pair ONE launch for both mixers through hip_ops.both(), up to PAIR_OWN_MAX_ROWS
# rows per mixer, where it is also faster on the device than the library's two GEMMs (DiffMa-L/2 widths, both mixers, us incl. launch,
# tools/bench_gemm_own.py: batch 8 in_proj 43 -> 21 forward, 42 -> 30 weight gradient, out_proj 41 -> 16 / 38 -> 15 / 40 -> 22; from
# ~6 000 rows the library's large tiles win).  Above that, and for shapes dm_gemm does not take: one plain library GEMM per mixer --
# the products the unpaired path has always issued, tuned and recorded (a batch-2 library GEMM is not safe here: DESIGN.md section 7).
PAIR_OWN_MAX_ROWS = int(os.environ.get("DIFFMA_PAIR_OWN_MAX_ROWS", "3200"))

# Large-batch projections on K12 (csrc/gemm_large.hip).  DIFFMA_GEMM_LARGE=0 (hip_ops.GEMM_LARGE) returns every product to the library.
# DIFFMA_GEMM_LARGE_MIN_COLS: K12 is taken from this many output columns.  Measured against the TunableOp-tuned library at M = 100 352
# (profiles/r05_gemm_large_ablation.txt, stand-alone): N = 2048 and 1024 level or ahead (in_proj forward 216 vs 222 us, out_proj
# input gradient 108 vs 125 / 148 us), N = 512 level (out_proj forward 104 vs 105) or behind (in_proj input gradient, K = 2048: 223 vs
# 198).  Inside the training step K12's launches run ~10 % longer than stand-alone and the step is 0.5 % SLOWER with K12 on the two
# wide products than with the library everywhere (220.1 vs 219.1 ms, same box; 221.9 with K12 on all four): at parity, not ahead.
# The default keeps it on the wide products; DIFFMA_GEMM_LARGE_MIN_COLS=512 puts all four on it.
LARGE_MIN_ROWS = int(os.environ.get("DIFFMA_GEMM_LARGE_MIN_ROWS", "12288"))
LARGE_MIN_COLS = int(os.environ.get("DIFFMA_GEMM_LARGE_MIN_COLS", "1024"))
LARGE_MAX_K_NARROW = int(os.environ.get("DIFFMA_GEMM_LARGE_MAX_K_NARROW", "1024"))     # for outputs narrower than 1024 columns
# dx = dy W as dy (W^T)^T with a transposed 16-bit weight copy (a few MB, one small launch): both operands then have the contraction
# index contiguous, and the library's NT kernels beat its NN kernels at these shapes.  Measured at M = 100 352
# (tools/bench_gemm_large.py): the library's NN form 217 / 148 us (in_proj / out_proj) against 198 / 125 us for its NT form and
# 223 / 108 us for K12.
LARGE_DGRAD_NT = os.environ.get("DIFFMA_DGRAD_NT", "1") == "1"

FWD, DGRAD, WGRAD = "fwd", "dgrad", "wgrad"
# the caller: one mixer's linear, the pair's linear, the operator's inner products (x_proj, dt_proj) for G = 2 or for G = 1
SINGLE, PAIR, INNER_PAIR, INNER_SINGLE = "single", "pair", "inner_pair", "inner_single"
OWN, LARGE, LIB, LIB_NT = "dm_gemm", "dm_gemm_large", "library", "library_nt"
_DM_GEMM_FORM = {FWD: (True, True, None), DGRAD: (True, False, None), WGRAD: (False, False, torch.float32)}   # a_kmajor, b_kmajor, out_dtype

# dm_gemm's row window per caller, (first row count, rows-per-mixer divisor): one product only from 64 rows (below that a GEMM is a
# handful of workgroups either way); the pair from the first row; the operator's inner products are a choice of the pair alone
# (64-column products: the own kernel holds up to ~4x the rows) -- the single mixer keeps them on the library.
_OWN_ROWS = {SINGLE: (64, 1), PAIR: (0, 1), INNER_PAIR: (0, 4)}


def own_rows(caller, M):
    first, div = _OWN_ROWS.get(caller, (None, 1))
    return first is not None and M >= first and M // div <= PAIR_OWN_MAX_ROWS


def large_shape(M, N, K):
    """K12's rule for C [M, N] = a [M, K] @ b [N, K]^T on plain values: rows, output columns, and a short contraction for narrow outputs."""
    return M >= LARGE_MIN_ROWS and N >= LARGE_MIN_COLS and not (N < 1024 and K > LARGE_MAX_K_NARROW)


def _large_takes(a, b):
    return large_shape(a.shape[0], b.shape[0], a.shape[1]) and hip_ops.gemm_large_supported(a, b)


def route(kind, caller, a, b, has_bias=False):
    """The kernel for one product of ONE mixer; a, b: its 2-D operands as in the module docstring (DGRAD: dy made contiguous)."""
    M = a.shape[0]
    if not has_bias and own_rows(caller, M) and hip_ops.gemm_supported(a, b, *_DM_GEMM_FORM[kind]):
        return OWN                       # small launches: faster than the library's quantised tile grid
    if caller != SINGLE:
        return LIB
    if kind == FWD and not has_bias and _large_takes(a, b):
        return LARGE                     # large batch: the persistent 256 x 256 kernel
    if kind == DGRAD and LARGE_DGRAD_NT and a.is_cuda and M >= LARGE_MIN_ROWS and a.dtype in (torch.bfloat16, torch.float16):
        # (b.t().contiguous() as far as gemm_large_supported looks: a fresh, so aligned, row-major [K, N] tensor)
        wt = SimpleNamespace(is_cuda=b.is_cuda, dtype=b.dtype, shape=tuple(b.shape[::-1]), dim=lambda: 2, stride=lambda i: (b.shape[0], 1)[i], data_ptr=lambda: 0)
        return LARGE if _large_takes(a, wt) else LIB_NT
    return LIB


def _own_pair(a, b, a_kmajor, b_kmajor, out, accumulate=False):
    """out[g] (+)= opA(a[g]) @ opB(b[g]) for g = 0, 1 in ONE launch (dm_gemm_n)."""
    hip_ops.both(lambda g: hip_ops.gemm(a[g], b[g], a_kmajor, b_kmajor, out=out[g], accumulate=accumulate))
    return out


def _library(kind, caller, a, b, bias=None, out=None, accumulate=False, nt=False, a_strided=None):
    """One mixer's product on the library, in the form its caller class has always issued."""
    if kind == WGRAD:
        return _tn_splitk(a, b)
    if kind == FWD:
        return GemmChain.run(torch.mm, a, b.t(), out=out) if caller == PAIR else GemmChain.run(F.linear, a, b, bias)
    if accumulate:          # in place: an out-of-place addmm first copies `out` into its result (a 2 x 308 MB device memcpy per call at x_proj)
        return GemmChain.run(out.addmm_, a, b)
    if caller == PAIR:
        return GemmChain.run(torch.mm, a, b, out=out)
    return GemmChain.run(F.linear, a, b.t().contiguous()) if nt else GemmChain.run(torch.mm, a if a_strided is None else a_strided, b)


def product(kind, caller, a, b, bias=None, has_bias=False, out=None, accumulate=False, a_strided=None):
    """Issue one product by its route.  SINGLE: a, b are the operands (FWD takes x with any leading dimensions and returns them); bias: the
    forward's; has_bias: a backward product of a linear that has one; a_strided: dy before it was made contiguous, which is what the library's
    small-batch input gradient has always read.  Every other caller: a, b (and out) hold G mixers' operands, [G, ...] tensors or sequences, and
    so does the result -- ONE dm_gemm launch for the pair, else one library product per mixer; accumulate: out += (DGRAD)."""
    ak, bk, od = _DM_GEMM_FORM[kind]
    if caller == SINGLE:
        a2 = a.reshape(-1, a.shape[-1])
        r = route(kind, SINGLE, a2, b, has_bias or bias is not None)
        if r in (LIB, LIB_NT):
            return _library(kind, SINGLE, a, b, bias, nt=r == LIB_NT, a_strided=a_strided)
        y = hip_ops.gemm(a2, b, ak, bk, out_dtype=od) if r == OWN else hip_ops.gemm_large(a2, b if kind == FWD else b.t().contiguous())
        return y.view(*a.shape[:-1], y.shape[-1]) if kind == FWD else y
    a0, b0 = a[0], b[0]
    r = route(kind, caller, a0, b0)
    if out is None and (r == OWN or (caller == PAIR and kind != WGRAD)):
        P, Q, _ = hip_ops._gemm_dims(a0, b0, ak, bk)
        out = torch.empty((len(a), P, Q), dtype=od or a0.dtype, device=a0.device)
    if r == OWN:
        return _own_pair(a, b, ak, bk, out, accumulate)
    res = [_library(kind, caller, a[g], b[g], out=None if out is None else out[g], accumulate=accumulate) for g in range(len(a))]
    return res if out is None else out


def _to(t, dtype):
    return t if t.dtype == dtype else t.to(dtype)


class _LinearSplitKFn(torch.autograd.Function):
    """F.linear whose weight gradient uses the split-K product above (the projections' dW GEMMs have K = B*L)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        dev = x.device.type
        dt_ = torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else x.dtype
        xc = _to(x, dt_)
        wc = cast_weight(weight, dt_)                    # the step's shadow copy when current (step_prep), else a cast
        ctx.save_for_backward(xc, wc)
        ctx.meta = (x.dtype, weight.dtype, None if bias is None else bias.dtype)
        return product(FWD, SINGLE, xc, wc, None if bias is None else cast_weight(bias, dt_))

    @staticmethod
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        x_dt, w_dt, b_dt = ctx.meta
        with torch.autocast(device_type=xc.device.type, enabled=False):
            dy2 = _to(dy.reshape(-1, dy.shape[-1]), xc.dtype)
            dy2c, x2c, has_bias = dy2.contiguous(), xc.reshape(-1, xc.shape[-1]).contiguous(), b_dt is not None
            dx = product(DGRAD, SINGLE, dy2c, wc, has_bias=has_bias, a_strided=dy2).view(xc.shape).to(x_dt) if ctx.needs_input_grad[0] else None
            dw = product(WGRAD, SINGLE, dy2c, x2c, has_bias=has_bias).to(w_dt) if ctx.needs_input_grad[1] else None
            db = dy2.sum(0, dtype=torch.float32).to(b_dt) if (has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db


def linear_splitk(x, weight, bias=None):
    """Drop-in for F.linear(x, weight, bias) on the token-major projections (in_proj / out_proj)."""
    return _LinearSplitKFn.apply(x, weight, bias)


def _as_pair(a, b):
    """[2, ...] tensor holding a and b: the shared buffer when they already are its two halves (no copy), else a stack."""
    if (a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
            and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size() and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()):
        return torch.as_strided(a, (2,) + tuple(a.shape), (a.numel(),) + tuple(a.stride()))
    return torch.stack([a, b])


class _LinearPairFn(torch.autograd.Function):
    """(x0 @ W0^T, x1 @ W1^T) as ONE dm_gemm launch each way; bias-free (in_proj / out_proj of the mixers, block/mamba.py:259-261,315)."""

    @staticmethod
    def forward(ctx, x0, x1, W0, W1):
        dev = x0.device.type
        dt_ = torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else x0.dtype
        xp = _as_pair(_to(x0, dt_), _to(x1, dt_))                                                         # [2, B, L, K]
        Wst = stacked_pair(W0, W1, dt_)                                                                   # [2, N, K]
        ctx.save_for_backward(xp, Wst)
        ctx.meta = (x0.dtype, W0.dtype)
        y = product(FWD, PAIR, xp.view(2, -1, xp.shape[-1]), Wst).view(2, *x0.shape[:-1], Wst.shape[1])
        return y[0], y[1]

    @staticmethod
    def backward(ctx, dy0, dy1):
        xp, Wst = ctx.saved_tensors
        x_dt, w_dt = ctx.meta
        with torch.autocast(device_type=xp.device.type, enabled=False):
            dy = _as_pair(_to(dy0.contiguous(), xp.dtype), _to(dy1.contiguous(), xp.dtype)).view(2, -1, Wst.shape[1])
            dx = _to(product(DGRAD, PAIR, dy, Wst).view(xp.shape), x_dt)
            dW = product(WGRAD, PAIR, dy, xp.view(2, -1, Wst.shape[2]))       # fp32 (on the library: the unpaired path's products)
            return dx[0], dx[1], _to(dW[0], w_dt), _to(dW[1], w_dt)


def linear_pair(x0, x1, W0, W1):
    """(F.linear(x0, W0), F.linear(x1, W1)) for the two mixers of a block: one launch per product, forward and backward."""
    return _LinearPairFn.apply(x0, x1, W0, W1)
