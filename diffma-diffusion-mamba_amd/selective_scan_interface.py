"""Reference-facing operators, backed by the gfx950 kernels (C ABI: include/diffma_hip.h).

Names, argument order and meaning mirror what the reference imports
    block/mamba.py:11   from mamba_ssm.ops.selective_scan_interface import selective_scan_fn, mamba_inner_fn
    block/mamba.py:13   from causal_conv1d import causal_conv1d_fn
so a maintainer can point those imports here.  Tensors arrive in the reference's
channel-major convention (B, D, L); internally everything is token-major [B, L, D] (channel stride 1),
which is what the lane-per-channel kernels want.  A (B, D, L)-shaped *view* of a token-major buffer is
consumed without a copy; a genuinely L-contiguous tensor is repacked once.

`spiral_ssm` is the fused 3-direction operator the DiffMa mixer uses (block/mamba.py:343-355): token
gather + conv1d + SiLU, x_proj, dt_proj, selective scan with the z gather and the CrossMerge
inverse reindex folded into row addressing, then the 3-way merge BEFORE out_proj.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _lib, hip_ops, projections as proj
from .projections import DGRAD, FWD, INNER_PAIR, INNER_SINGLE, SINGLE, WGRAD, GemmChain, linear_pair, linear_splitk, product     # noqa: F401 (GemmChain, linear_pair: public here)
from .step_prep import cast_weight, stacked_pair


REPACK_OWN = os.environ.get("DIFFMA_REPACK_OWN", "1") == "1"        # 0: the ATen strided copy again (A/B runs)


def _repack_own(t: torch.Tensor) -> bool:
    """dm_repack takes the tensor: a contiguous-last-axis 3-d device tensor of a supported dtype whose batch fits the launch grid's
    z extent (65 535; larger stacked batches keep the ATen strided copy, which has no such limit)."""
    return (REPACK_OWN and t.is_cuda and t.dim() == 3 and t.stride(2) == 1 and t.shape[0] <= 65535
            and t.dtype in (torch.float32, torch.bfloat16, torch.float16))


def _to_token_major(t: torch.Tensor) -> torch.Tensor:
    """(B, D, L) in any layout -> a [B, L, D] tensor with stride(-1) == 1 (no copy when possible; a genuinely L-contiguous
    tensor -- what the reference hands over, block/mamba.py:333-348 -- goes through dm_repack).  No autograd: callers are
    autograd Functions' forward / backward bodies; `_RepackFn` is the differentiable form."""
    tm = t.transpose(1, 2)
    if tm.stride(-1) == 1:
        return tm
    if _repack_own(t):
        return hip_ops.repack(t, True)
    return tm.contiguous()


def _to_channel_major(t: torch.Tensor) -> torch.Tensor:
    """[B, L, D] token-major -> a CONTIGUOUS (B, D, L) tensor (the layout the reference's glue goes on with: CrossScan.backward,
    the in_proj gradient products, block/mamba.py:47-57, 333-337); a lazily transposed view would make every consumer a
    strided ATen copy."""
    if _repack_own(t):
        return hip_ops.repack(t, False)
    return t.transpose(1, 2).contiguous()


class _RepackFn(torch.autograd.Function):
    """(B, D, L) channel-major -> [B, L, D] token-major with the gradient handed back channel-major and contiguous."""

    @staticmethod
    def forward(ctx, t):
        return _to_token_major(t)

    @staticmethod
    def backward(ctx, g):
        if g.stride(-1) != 1:
            g = g.contiguous()
        return _to_channel_major(g)


def _bc_token_major(Bm: torch.Tensor):
    """B/C arrive as (B, N, L) or (B, G, N, L); return ([B, L, G*N] with state stride 1, G)."""
    if Bm.dim() == 3:
        Bm = Bm[:, None]
    bsz, G, N, L = Bm.shape
    t = Bm.permute(0, 3, 1, 2)                                  # (B, L, G, N)
    if not (t.stride(3) == 1 and t.stride(2) == N):
        t = t.contiguous()
    return t.reshape(bsz, L, G * N) if t.is_contiguous() else t.as_strided((bsz, L, G * N), (t.stride(0), t.stride(1), 1)), G


class _SelectiveScanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, delta, A, Bm, Cm, D, z, delta_bias, delta_softplus, return_last_state, grad_on=True):
        ut, dt = _to_token_major(u), _to_token_major(delta)
        zt = _to_token_major(z) if z is not None else None
        if dt.dtype != ut.dtype:
            dt = dt.to(ut.dtype)
        if zt is not None and zt.dtype != ut.dtype:
            zt = zt.to(ut.dtype)
        Bt, G = _bc_token_major(Bm)
        Ct, _ = _bc_token_major(Cm)
        if Bt.dtype not in (torch.float32, ut.dtype):
            Bt = Bt.to(ut.dtype)
        if Ct.dtype != Bt.dtype:
            Ct = Ct.to(Bt.dtype)
        S, L, Dm = ut.shape
        N = A.shape[1]
        # grad_on = the caller's grad mode (inside forward() it is always off): no checkpoints under torch.no_grad()
        need_grad = grad_on and any(t is not None and t.requires_grad for t in (u, delta, A, Bm, Cm, D, z, delta_bias))
        ckpt = None
        if need_grad:
            ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, ut.dtype, ut.device)
        last = torch.empty((S, N, Dm), dtype=torch.float32, device=ut.device) if return_last_state else None
        out = hip_ops.scan_fwd(ut, dt, A, Bt, Ct, D, zt, delta_bias, delta_softplus, ckpt=ckpt, last_state=last,
                               ngroups=G)
        ctx.delta_softplus = delta_softplus
        ctx.G = G
        ctx.has_z, ctx.has_D, ctx.has_bias = z is not None, D is not None, delta_bias is not None
        ctx.b4, ctx.c4 = Bm.dim() == 4, Cm.dim() == 4
        ctx.save_for_backward(ut, dt, A, Bt, Ct, D, zt, delta_bias, ckpt)
        out_cm = out.transpose(1, 2)                            # (B, D, L) view, like the reference returns
        if return_last_state:
            ctx.mark_non_differentiable(last)
            return out_cm, last.transpose(1, 2)
        return out_cm

    @staticmethod
    def backward(ctx, dout, *ignored):
        ut, dt, A, Bt, Ct, D, zt, delta_bias, ckpt = ctx.saved_tensors
        if ctx.G != 1:
            raise NotImplementedError("backward with ngroups > 1 is not wired (DiffMa uses ngroups = 1)")
        dot = _to_token_major(dout)
        if dot.dtype != ut.dtype:
            dot = dot.to(ut.dtype)
        du, ddelta, dz, dB, dC, dA, dD, dbias = hip_ops.scan_bwd(ut, dt, A, Bt, Ct, D, zt, delta_bias, dot, ckpt,
                                                                 ctx.delta_softplus)
        cm = lambda t: t.transpose(1, 2)
        dBm = dB.to(Bt.dtype).transpose(1, 2)                   # (B, N, L)
        dCm = dC.to(Ct.dtype).transpose(1, 2)
        if ctx.b4:
            dBm = dBm[:, None]
        if ctx.c4:
            dCm = dCm[:, None]
        return (cm(du), cm(ddelta), dA.to(A.dtype), dBm, dCm,
                dD.to(D.dtype) if ctx.has_D else None, cm(dz) if ctx.has_z else None,
                dbias.to(delta_bias.dtype) if ctx.has_bias else None, None, None, None)


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
                      return_last_state=False):
    """Drop-in for mamba_ssm's selective_scan_fn (imported at block/mamba.py:11).

    u, delta, z: (B, D, L); A: (D, N) real; B, C: (B, N, L) or (B, G, N, L) (input-dependent);
    D, delta_bias: (D,) fp32.  Returns out (B, D, L) [, last_state (B, D, N)].
    """
    if A.is_complex():
        raise NotImplementedError("complex A is not supported (DiffMa uses the real S4D-real init, block/mamba.py:304-310)")
    if B.dim() not in (3, 4) or C.dim() not in (3, 4):
        raise NotImplementedError("only input-dependent B/C are supported (the only mode DiffMa uses)")
    return _SelectiveScanFn.apply(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, torch.is_grad_enabled())


class _CausalConv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, silu):
        xt = _to_token_major(x)
        out = hip_ops.gather_conv1d_fwd(xt, weight, bias, silu=silu)
        ctx.silu = silu
        ctx.save_for_backward(xt, weight, bias)
        return out.transpose(1, 2)

    @staticmethod
    def backward(ctx, dout):
        xt, weight, bias = ctx.saved_tensors
        dot = _to_token_major(dout)
        if dot.dtype != xt.dtype:
            dot = dot.to(xt.dtype)
        dx, dw, db = hip_ops.gather_conv1d_bwd(xt, weight, bias, dot, silu=ctx.silu)
        return dx.transpose(1, 2), dw.to(weight.dtype).reshape(weight.shape), (db.to(bias.dtype) if bias is not None else None), None


def causal_conv1d_fn(x, weight, bias=None, seq_idx=None, initial_states=None, return_final_states=False,
                     final_states_out=None, activation=None):
    """Drop-in for causal_conv1d.causal_conv1d_fn (imported at block/mamba.py:13).  x: (B, D, L), weight (D, W)."""
    if activation not in (None, "silu", "swish"):
        raise NotImplementedError("activation must be None, silu or swish")
    if seq_idx is not None or initial_states is not None or return_final_states or final_states_out is not None:
        raise NotImplementedError("seq_idx / initial_states / final_states are decode-time features DiffMa never uses")
    return _CausalConv1dFn.apply(x, weight, bias, activation is not None)


# ------------------------------------------------------------------------------------------------
# The TWO mixers of a DiffMa block as one set of launches (reference block/mamba_block.py:107-108)
# ------------------------------------------------------------------------------------------------
# The reference runs mamba1(x_ssm) and mamba2(w_ssm) one after the other: same shapes, different weights and spiral tables.  Its own
# configuration trains at ONE sample per GPU (config/brain.yaml:11), where a step is bound by the number of kernel launches (eager:
# the host's launch rate; hipGraph: ~8 us of dispatch per node), not by what the kernels do.  The pair path issues every stage once
# for both mixers: the projections through projections.linear_pair / `product`, the kernels through hip_ops.both() -> the `_n` entry
# points of the C ABI (one grid, blockIdx.z picks the mixer).  Arithmetic per mixer is unchanged: kernels bit-identical, GEMMs to
# library rounding.  Used for small launches only (below the fused conv + x_proj threshold); large batches gain nothing from it.
PAIR_MIXERS = os.environ.get("DIFFMA_PAIR_MIXERS", "1") == "1"


# ------------------------------------------------------------------------------------------------
# Fused 3-direction operator of the DiffMa mixer: one mixer, or the two mixers of a block in one set of launches
# ------------------------------------------------------------------------------------------------
# DIFFMA_HOIST_GATE=0: gate (and softplus) back inside every per-direction scan, as upstream evaluates them (A/B runs, tests)
HOIST_GATE = os.environ.get("DIFFMA_HOIST_GATE", "1") == "1"


class _SpiralSSMFn(torch.autograd.Function):
    """xz [B, L, 2*Din] token-major -> merged pre-projection output y [B, L, Din], for G = 1 mixer or for the G = 2 mixers of a block
    at once.  The per-mixer operands arrive field by field, G of each; every kernel stage runs through `stage`: hip_ops.both for the
    pair (ONE launch for both mixers), the plain call for one mixer.  Results that the pair shares as halves of one allocation
    (xc, x_dbl, y, pre, du, dx_dbl, dxz) are [G, ...] buffers either way.

    scan_index [ndir, L]: position l of direction k reads token scan_index[k][l]   (CrossScan, block/mamba.py:41-45)
    Because CrossMerge adds direction k's output row origina_k[t] at token t and origina_k is the inverse
    permutation of scan_index[k] (tools.py:38-42), step l's result belongs to token scan_index[k][l]: the
    same table drives the gather of x and z and the scatter of y.

    The pair (spiral_ssm_pair_supported) is one arm of what follows: hoisted gate + hoisted softplus, unfused conv, 16-bit I/O,
    d_state 16, small launches.
    """
    NFIELD = 9             # xz, scan_index, conv_w, conv_b, Wx, Wdt, dt_bias, A, Dskip

    @staticmethod
    def _stage(G):
        return hip_ops.both if G == 2 else (lambda fn: (fn(0),))

    @staticmethod
    def forward(ctx, grad_on, out_index, merge, G, defer, *ops):
        """out_index (default: scan_index): row of the per-direction output that step l's result is written to -- the
        baseline blocks need a scatter that is not the gather's inverse (ViM, block/mamba.py:362-367).  merge=False returns
        the per-direction outputs [ndir, B, L, Din] instead of their sum.  Returns a tuple of G outputs.
        defer (a _GateDefer or None; one mixer): the caller offers to run the hoisted gate's backward inside out_proj's input
        gradient (_GatedOutProjFn).  Taken when the gate is hoisted and a backward will run: the outputs are then (y, pre), y not
        differentiable, and the gradient that arrives for `pre` IS g = dy * silu(z)."""
        xz, idx, cw, cb, Wx, Wdt, bias, A, Dk = (ops[i * G:(i + 1) * G] for i in range(_SpiralSSMFn.NFIELD))
        stage, each, inner = _SpiralSSMFn._stage(G), range(G), (INNER_PAIR if G == 2 else INNER_SINGLE)
        Bsz, L, D2 = xz[0].shape
        Din = D2 // 2
        ndir = idx[0].shape[0]
        R, N = Wdt[0].shape[1], A[0].shape[1]
        S, M = ndir * Bsz, ndir * Bsz * L
        dt_, dev = xz[0].dtype, xz[0].device
        need_grad = grad_on and any(ctx.needs_input_grad)                      # grad_on: the caller's grad mode
        # kept for the backward, indexed by mixer: the pair's shared shadow buffer (no launch), else the step's shadow or one cast per step
        if G == 2:
            Wx_c, Wdt_c = stacked_pair(Wx[0], Wx[1], dt_), stacked_pair(Wdt[0], Wdt[1], dt_)    # [2, R+2N, Din], [2, Din, R]
        else:
            Wx_c, Wdt_c = cast_weight(Wx[0], dt_)[None], cast_weight(Wdt[0], dt_)[None]
        if hip_ops.conv_xproj_supported(xz[0][..., :Din], Wx_c[0], S, cw[0].shape[-1]):
            # gather + conv + SiLU + x_proj in one kernel: x~ is projected while its tile is still on the CU
            xc, x_dbl = zip(*stage(lambda g: hip_ops.gather_conv1d_xproj_fwd(xz[g][..., :Din], cw[g], cb[g], Wx_c[g], row_index=idx[g],
                                                                             ndir=ndir, silu=True)))
        else:
            xc = torch.empty((G, S, L, Din), dtype=dt_, device=dev)
            stage(lambda g: hip_ops.gather_conv1d_fwd(xz[g][..., :Din], cw[g], cb[g], row_index=idx[g], ndir=ndir, silu=True, out=xc[g]))
            # x_proj on the library is one product per mixer: as a batch-2 GEMM its [M, 1024] x [1024, 64] shape makes TunableOp's first-use
            # tuning run a library candidate that faults (MI355X, ROCm 7.2: memory access fault inside the tuning loop)
            x_dbl = product(FWD, inner, xc.view(G, M, Din), Wx_c)                                             # G x [ndir*B*L, R+2N]
        # Hoisted gate: CrossScan permutes x and z together and CrossMerge applies the inverse permutation (block/mamba.py:41-45,
        # 66-68), so merged[t] = silu(z[t]) * sum_k y~_k[t]: the scans run WITHOUT z and the gate is applied once per token by the
        # merge (one z read in an HBM-bound kernel) instead of three times inside the VALU-bound scans.  Needs the scatter table
        # to be the gather table (not ViM's) and a merge to ride on.
        # One direction (the reference's own three-calls-per-mixer pattern through mamba_inner_fn, the ZigMa order): the gate pass is an
        # extra launch, worth it only where the scans are VALU-bound -- the large launches (K2 1 058 -> ~830 us per 512 sequences).
        hoist = HOIST_GATE and merge and out_index is None and (ndir > 1 or Bsz >= hip_ops.XPROJ_FUSED_MIN_SEQS)
        # Hoisted softplus: delta = softplus(dt_proj(.) + bias) leaves the dt_proj kernel activated (csrc/dtproj.hip) and the scans
        # run with DM_FLAG_DELTA_ACTIVATED (forward: nothing to evaluate; backward: only 1 - exp(-delta)).
        # The backward of that flag exists for d_state 16 only (csrc/scan_bwd.hip): other widths keep the softplus inside the scans.
        act = hoist and N == 16 and hip_ops.dtproj_softplus_supported(x_dbl[0], Wdt_c[0])
        assert G == 1 or act, "the pair path is built for the hoisted gate with the activated delta (spiral_ssm_pair_supported)"
        if act:
            delta = stage(lambda g: hip_ops.dtproj_softplus_fwd(x_dbl[g], Wdt_c[g], bias[g]).view(S, L, Din))
        else:
            delta = [t.view(S, L, Din) for t in product(FWD, INNER_SINGLE, [t[:, :R] for t in x_dbl], Wdt_c)]
        ckpt = [hip_ops.alloc_scan_ckpt(S, L, N, Din, dt_, dev) if need_grad else None for _ in each]
        oidx = idx if out_index is None else (out_index,)
        xd3 = [t.view(S, L, R + 2 * N) for t in x_dbl]
        ydir = stage(lambda g: hip_ops.scan_fwd(                               # token order; gated here unless the merge does it
            xc[g], delta[g], A[g], xd3[g][..., R:R + N], xd3[g][..., R + N:], Dk[g], None if hoist else xz[g][..., Din:], bias[g], True,
            z_row_index=idx[g], out_row_index=oidx[g], batch_per_dir=Bsz, ckpt=ckpt[g], delta_activated=act))
        pre = None
        if hoist:
            y = torch.empty((G, Bsz, L, Din), dtype=dt_, device=dev)
            pre = torch.empty((G, Bsz, L, Din), dtype=dt_, device=dev) if need_grad else None          # ungated sum, kept for dz
            stage(lambda g: hip_ops.token_merge(ydir[g].view(ndir, Bsz, L, Din), gate=xz[g][..., Din:],
                                                pre_out=None if pre is None else pre[g], out=y[g]))
            out = tuple(y)
            if defer is not None:
                defer.taken = G == 1 and pre is not None
                if defer.taken:
                    out = (y[0], pre[0])
                    ctx.mark_non_differentiable(y[0])
                    ctx.set_materialize_grads(False)          # (no zero-filled gradient for y)
        elif not merge:
            out = tuple(t.view(ndir, Bsz, L, Din) for t in ydir)
        else:
            out = tuple(hip_ops.token_merge(t.view(ndir, Bsz, L, Din)) if ndir > 1 else t for t in ydir)
        if need_grad:
            ctx.save_for_backward(*xz, *idx, *oidx, *cw, *cb, *bias, *A, *Dk, *xc, *x_dbl, *delta, *ckpt,
                                  *((None,) * G if pre is None else pre), Wx_c, Wdt_c)
            ctx.meta = (G, merge, hoist, act, Wx[0].dtype, Wdt[0].dtype)
            ctx.defer = defer if (defer is not None and defer.taken) else None
        return out

    @staticmethod
    def backward(ctx, *dys):
        G, merge, hoist, act, wx_dt, wdt_dt = ctx.meta
        sv = ctx.saved_tensors
        xz, idx, oidx, cw, cb, bias, A, Dk, xc, x_dbl, delta, ckpt, pre = (sv[i * G:(i + 1) * G] for i in range(13))
        Wx_c, Wdt_c = sv[-2:]
        stage, each, inner = _SpiralSSMFn._stage(G), range(G), (INNER_PAIR if G == 2 else INNER_SINGLE)
        Bsz, L, D2 = xz[0].shape
        Din = D2 // 2
        ndir = idx[0].shape[0]
        R, N = Wdt_c.shape[2], A[0].shape[1]
        S, M = ndir * Bsz, ndir * Bsz * L
        dt_, dev = xz[0].dtype, xz[0].device
        defer = ctx.defer
        if defer is not None:
            # out_proj's backward has run the gate's backward: dys[1] is g, and the z half of d(xz) is written in its buffer
            assert dys[1] is not None and defer.dxz is not None, "the deferred gate backward did not run"
            gy, dxz, defer.dxz = [dys[1].contiguous().to(dt_)], defer.dxz, None
        else:
            dy = [t.contiguous().to(dt_) for t in dys]
            if not merge:
                dy = [t.view(S, L, Din) for t in dy]       # one gradient per direction
            dxz = torch.empty((G, Bsz, L, D2), dtype=dt_, device=dev)
        dx_dbl = torch.empty((G, M, R + 2 * N), dtype=dt_, device=dev)
        du = torch.empty((G, S, L, Din), dtype=dt_, device=dev)
        xd3 = [t.view(S, L, R + 2 * N) for t in x_dbl]
        if defer is not None:
            pass
        elif hoist:
            # the gate's backward once per token: g = dy * silu(z) is what the three directions read as their output gradient,
            # dz = dy * pre * silu'(z) goes straight into the z half of d(xz) (no dz slabs, no 3-slab merge)
            gy = stage(lambda g: hip_ops.gate_bwd(dy[g], xz[g][..., Din:], pre[g], dz_out=dxz[g][..., Din:])[0])
        else:
            gy = dy
        res = stage(lambda g: hip_ops.scan_bwd(
            xc[g], delta[g], A[g], xd3[g][..., R:R + N], xd3[g][..., R + N:], Dk[g], None if hoist else xz[g][..., Din:], bias[g], gy[g],
            ckpt[g], True, z_row_index=idx[g], out_row_index=oidx[g], batch_per_dir=Bsz, dout_per_seq=not merge, du_out=du[g],
            dbc_out=dx_dbl[g].view(S, L, R + 2 * N)[..., R:], delta_activated=act))        # dB | dC land in their x_dbl columns
        ddelta = [r[1].view(M, Din) for r in res]
        if hip_ops.dtproj_bwd_supported(ddelta[0], x_dbl[0], Wdt_c[0], dx_dbl[0]):
            # both consumers of ddelta -- the dt columns of d(x_dbl) and dW_dt -- in ONE read of it (csrc/dtproj.hip, K8b)
            dWdt = stage(lambda g: hip_ops.dtproj_bwd(ddelta[g], x_dbl[g], Wdt_c[g], dx_dbl[g]))
        else:
            for g, t in enumerate(product(DGRAD, INNER_SINGLE, ddelta, Wdt_c)):
                dx_dbl[g][:, :R] = t                   # (a strided `out=` is an untuned GEMM shape class: pathologically slow by default)
            dWdt = product(WGRAD, INNER_SINGLE, ddelta, [t[:, :R] for t in x_dbl])    # [Din, R]; the dt columns of x_dbl in place (leading dimension R + 2N)
        dWx = product(WGRAD, inner, dx_dbl, [t.view(M, Din) for t in xc])                                        # [R+2N, Din] fp32 each
        if hip_ops.conv_xproj_bwd_supported(xz[0][..., :Din], Wx_c[0], S, cw[0].shape[-1], du[0], dx_dbl[0]):
            # d x~ = du + dx_dbl @ Wx is formed tile by tile inside the conv backward (K4x) instead of by an addmm over [M, Din]
            merged_dx = hip_ops.DX_MERGED and cw[0].shape[-1] == 4      # one direction: dx straight into d(xz), no copy pass
            cres = stage(lambda g: hip_ops.gather_conv1d_xproj_bwd(xz[g][..., :Din], cw[g], cb[g], du[g], dx_dbl[g], Wx_c[g].t().contiguous(),
                                                                   row_index=idx[g], ndir=ndir, silu=True,
                                                                   merged_out=dxz[g][..., :Din] if merged_dx else None))
        else:
            merged_dx = False
            product(DGRAD, inner, dx_dbl, Wx_c, out=du.view(G, M, Din), accumulate=True)    # d x~ = du + dx_dbl @ Wx, in place
            cres = stage(lambda g: hip_ops.gather_conv1d_bwd(xz[g][..., :Din], cw[g], cb[g], du[g], row_index=idx[g], ndir=ndir, silu=True))
        if not merged_dx:                                          # K4x already summed the directions into dxz[..., :Din]
            stage(lambda g: hip_ops.token_merge(cres[g][0].view(ndir, Bsz, L, Din), out=dxz[g][..., :Din]))
        if not hoist:
            stage(lambda g: hip_ops.token_merge(res[g][2].view(ndir, Bsz, L, Din), out=dxz[g][..., Din:]))
        grads = (dxz, (None,) * G,
                 [cres[g][1].to(cw[g].dtype).reshape(cw[g].shape) for g in each],
                 [cres[g][2].to(cb[g].dtype) if cb[g] is not None else None for g in each],
                 [t.to(wx_dt) for t in dWx], [t.to(wdt_dt) for t in dWdt],
                 [res[g][7].to(bias[g].dtype) for g in each], [res[g][5].to(A[g].dtype) for g in each],
                 [res[g][6].to(Dk[g].dtype) for g in each])
        return (None, None, None, None, None) + tuple(t for field in grads for t in field)


def spiral_ssm_pair_supported(Bsz, L, dtype, mix0, mix1):
    """The call pattern the pair path is built for: two Mamba-1 mixers of equal shape on a ROCm device, 16-bit activations,
    d_state 16, a conv with bias, and a launch small enough that the unfused conv / chunk-parallel scans serve it."""
    if not (PAIR_MIXERS and HOIST_GATE and dtype in (torch.bfloat16, torch.float16)):
        return False
    idx0, idx1 = mix0.scan_index, mix1.scan_index
    if not idx0.is_cuda or idx0.shape != idx1.shape or idx0.shape[0] < 2 or idx0.shape[1] != L:
        return False
    if mix0.A_log.shape != mix1.A_log.shape or mix0.A_log.shape[1] != 16 or mix0.conv1d.bias is None or mix1.conv1d.bias is None:
        return False
    if mix0.conv1d.weight.shape != mix1.conv1d.weight.shape or mix0.x_proj.weight.shape != mix1.x_proj.weight.shape:
        return False
    if idx0.shape[0] * Bsz >= hip_ops.XPROJ_FUSED_MIN_SEQS:
        return False
    Din, R = mix0.dt_proj.weight.shape
    code = {torch.bfloat16: _lib.DM_BF16, torch.float16: _lib.DM_F16}[dtype]
    return bool(hip_ops.DTPROJ_FUSED and (R + 2 * 16) % 8 == 0 and _lib.load().dm_dtproj_softplus_supported(int(Din), int(R), code))


def spiral_ssm_pair(xz0, xz1, mix0, mix1, A0, A1):
    """The fused 3-direction operator (spiral_ssm) for the two mixers of a block in one set of launches."""
    per = lambda f: (f(mix0), f(mix1))
    with torch.autocast(device_type="cuda", enabled=False):
        return _SpiralSSMFn.apply(torch.is_grad_enabled(), None, True, 2, None, xz0, xz1, *per(lambda m: m.scan_index),
                                  *per(lambda m: m.conv1d.weight), *per(lambda m: m.conv1d.bias), *per(lambda m: m.x_proj.weight),
                                  *per(lambda m: m.dt_proj.weight), *per(lambda m: m.dt_proj.bias.float()), A0.float(), A1.float(),
                                  *per(lambda m: m.D.float()))


# ------------------------------------------------------------------------------------------------
# Mamba-2 mixer
# ------------------------------------------------------------------------------------------------
class _SpiralSSDFn(torch.autograd.Function):
    """The Mamba-2 mixer between in_proj and out_proj as ONE autograd node: zxbcdt [B, L, 2*Din + 2N + H] (token-major
    in_proj output, column blocks [z | x | B | C | dt], block/mamba2.py:380-400) -> gated, RMS-normalised, merged y [B, L, Din].
    The backward assembles d(zxbcdt) in place from the kernels' outputs (no slice/cat/index autograd nodes, no zero fills)."""

    @staticmethod
    def forward(ctx, zxbcdt, conv_w, conv_b, dt_bias_h, A_h, D_h, norm_w, eps, scan_index, scan_index_inv, Din, N, grad_on=True):
        Bsz, L, _ = zxbcdt.shape
        H = A_h.shape[0]
        P = Din // H
        ndir = scan_index.shape[0]
        S, Cx = ndir * Bsz, Din + 2 * N
        z, xbc_in, dt_tok = zxbcdt[..., :Din], zxbcdt[..., Din:Din + Cx], zxbcdt[..., Din + Cx:]
        xBC = hip_ops.gather_conv1d_fwd(xbc_in, conv_w, conv_b, row_index=scan_index, ndir=ndir, silu=True)        # [S, L, Cx]
        x, Bm, Cm = xBC[..., :Din], xBC[..., Din:Din + N], xBC[..., Din + N:]
        need_grad = grad_on and any(ctx.needs_input_grad[:7])
        ctx.ssd = False
        if hip_ops.ssd_fwd_supported(xBC, L, P, N, views=(x, Bm, Cm), gate=z) and (not need_grad or hip_ops.ssd_bwd_supported(xBC, L, P, N, gate=z)):
            # the matrix pipe (csrc/ssd.hip, ssd_bwd.hip, ssd_bwd_wide.hip): single-chunk SSD as dense tile products per (sequence,
            # head), the per-head dt read in the kernel through the gather table -- no [S, L, Din] delta tensor, no per-state
            # recurrence, and nothing but the operands saved for the backward (which recomputes the score tiles).  At d_state 16 the
            # backward is on by default; at the wide states of hip_ops.SSD_FWD_WIDTHS a no-grad call comes here, and a call that
            # needs gradients does only with hip_ops.SSD_MFMA_BWD_WIDE on (dm_ssd_bwd_wide) -- by default it takes the scan pair
            ydir = hip_ops.ssd_fwd(x, Bm, Cm, dt_tok, z, A_h, D_h, dt_bias_h, z_row_index=scan_index, out_row_index=scan_index,
                                   batch_per_dir=Bsz)
            out, rstd = _SpiralSSDFn._norm_merge(ydir, norm_w, eps, ndir, Bsz, L, Din)
            if need_grad:
                ctx.ssd = True
                ctx.save_for_backward(zxbcdt, conv_w, conv_b, xBC, ydir, rstd, norm_w, scan_index, A_h, D_h, dt_bias_h)
                ctx.meta = (Din, N, H, P, eps, dt_bias_h.dtype, A_h.dtype, D_h.dtype)
            return out
        if (not need_grad and hip_ops.ssd_fwd_supported(xBC, 1, P, N, views=(x, Bm, Cm), gate=z)      # (L = 1: everything but the length)
                and hip_ops.ssd_fwd_chunked_supported(xBC, L, P, N, views=(x, Bm, Cm), gate=z)):
            # turned down above for its length only (L > 224) and no gradients needed: the chunked matrix-pipe forward
            # (csrc/ssd_chunked.hip) instead of the scan; a call that needs gradients goes on to the scan pair below
            ydir = hip_ops.ssd_fwd_chunked(x, Bm, Cm, dt_tok, z, A_h, D_h, dt_bias_h, z_row_index=scan_index, out_row_index=scan_index,
                                           batch_per_dir=Bsz)
            return _SpiralSSDFn._norm_merge(ydir, norm_w, eps, ndir, Bsz, L, Din)[0]
        # dt is produced per token and per head: gather its rows per direction, broadcast head -> channels
        idx64 = scan_index.long()
        dt_g = torch.stack([dt_tok[:, idx64[k]] for k in range(ndir)])                                            # [ndir, B, L, H]
        delta = dt_g.reshape(S, L, H, 1).expand(S, L, H, P).reshape(S, L, Din)
        A = A_h.float().repeat_interleave(P)[:, None].expand(Din, N).contiguous()
        Dskip = D_h.float().repeat_interleave(P)
        dt_bias = dt_bias_h.float().repeat_interleave(P)
        ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Din, zxbcdt.dtype, zxbcdt.device) if need_grad else None
        ydir = hip_ops.scan_fwd(x, delta, A, Bm, Cm, Dskip, z, dt_bias, True, z_row_index=scan_index, out_row_index=scan_index,
                                batch_per_dir=Bsz, ckpt=ckpt, a_shared=True)     # token order, gated; one decay per head
        out, rstd = _SpiralSSDFn._norm_merge(ydir, norm_w, eps, ndir, Bsz, L, Din)
        ctx.save_for_backward(zxbcdt, conv_w, conv_b, xBC, ydir, rstd, norm_w, scan_index, delta, A, Dskip, dt_bias, ckpt, scan_index_inv)
        ctx.meta = (Din, N, H, P, eps, dt_bias_h.dtype, A_h.dtype, D_h.dtype)
        return out

    @staticmethod
    def _norm_merge(ydir, norm_w, eps, ndir, Bsz, L, Din):
        """Gated RMSNorm of every direction + merge; norm_w None (the operator called with rmsnorm_weight=None, one direction):
        the gated scan output itself."""
        if norm_w is None:
            if ndir != 1:
                raise NotImplementedError("the un-normalised Mamba-2 core is wired for one direction (the reference-facing operator)")
            return ydir.view(Bsz, L, Din), None
        return hip_ops.rmsnorm_merge_fwd(ydir.view(ndir, Bsz, L, Din), norm_w, eps)

    @staticmethod
    def _norm_merge_bwd(ydir, norm_w, eps, rstd, dout, ndir, Bsz, L, Din):
        if norm_w is None:
            return dout.contiguous().view(1, Bsz, L, Din), None
        return hip_ops.rmsnorm_merge_bwd(ydir.view(ndir, Bsz, L, Din), norm_w, eps, rstd, dout)

    @staticmethod
    def backward(ctx, dout):
        zxbcdt, conv_w, conv_b, xBC, ydir, rstd, norm_w, scan_index, *arm = ctx.saved_tensors
        Din, N, H, P, eps, bias_dt, A_dt, D_dt = ctx.meta
        Bsz, L, _ = zxbcdt.shape
        ndir = scan_index.shape[0]
        S, Cx = ndir * Bsz, Din + 2 * N
        dt_ = zxbcdt.dtype
        if dout.dtype != dt_:
            dout = dout.to(dt_)
        dyd, dnorm_w = _SpiralSSDFn._norm_merge_bwd(ydir, norm_w, eps, rstd, dout, ndir, Bsz, L, Din)                # [ndir, B, L, Din]
        dxBC = torch.empty((S, L, Cx), dtype=dt_, device=zxbcdt.device)
        x, Bm, Cm = xBC[..., :Din], xBC[..., Din:Din + N], xBC[..., Din + N:]
        # either arm fills dxBC and yields dz per direction, the d dt columns in token order and the per-head dA, dD, d dt_bias
        if ctx.ssd:
            A_h, D_h, dt_bias_h = arm
            _, dzs, dbc, ddt, dad = hip_ops.ssd_bwd(
                x, Bm, Cm, zxbcdt[..., Din + Cx:], zxbcdt[..., :Din], dyd.view(S, L, Din), A_h, D_h, dt_bias_h, z_row_index=scan_index,
                out_row_index=scan_index, batch_per_dir=Bsz, dx_out=dxBC[..., :Din])
            dxBC[..., Din:].copy_(dbc)                                                    # dB | dC (summed over the heads) in their xBC columns
            ddt4 = ddt.view(ndir, Bsz, L, H)                                              # already in token order, raw-dt gradient: add the directions
            ddt_tok = ddt4[0] if ndir == 1 else ddt4.sum(0)
            dA_h, dD_h, dbias_h = dad
        else:
            delta, A, Dskip, dt_bias, ckpt, scan_index_inv = arm
            _, ddelta, dzs, _, _, dA, dD, dbias = hip_ops.scan_bwd(
                x, delta, A, Bm, Cm, Dskip, zxbcdt[..., :Din], dt_bias, dyd.view(S, L, Din), ckpt, True, z_row_index=scan_index,
                out_row_index=scan_index, batch_per_dir=Bsz, dout_per_seq=True, du_out=dxBC[..., :Din], a_shared=True,
                dbc_out=dxBC[..., Din:])                                             # dB | dC land in their xBC columns
            # d(dt): sum the head's channels, put every direction back in token order (adjoint of the row gather), add the directions
            # (a matrix-vector product: the generic inner-dimension reduction kernel takes 150 us for this shape, the GEMV 20)
            ddt = torch.mv(ddelta.view(S * L * H, P), torch.ones(P, dtype=dt_, device=zxbcdt.device)).view(ndir, Bsz, L, H)
            inv64 = scan_index_inv.long()
            ddt_tok = ddt[0][:, inv64[0]].float()
            for k in range(1, ndir):
                ddt_tok = ddt_tok + ddt[k][:, inv64[k]].float()
            dA_h, dD_h, dbias_h = dA.view(H, P * N).sum(-1), dD.view(H, P).sum(-1), dbias.view(H, P).sum(-1)
        dx_slabs, dconv_w, dconv_b = hip_ops.gather_conv1d_bwd(zxbcdt[..., Din:Din + Cx], conv_w, conv_b, dxBC, row_index=scan_index,
                                                               ndir=ndir, silu=True)                              # token order
        dzx = torch.empty_like(zxbcdt)
        hip_ops.token_merge(dzs.view(ndir, Bsz, L, Din), out=dzx[..., :Din])
        hip_ops.token_merge(dx_slabs.view(ndir, Bsz, L, Cx), out=dzx[..., Din:Din + Cx])
        dzx[..., Din + Cx:].copy_(ddt_tok)
        return (dzx, dconv_w.to(conv_w.dtype).reshape(conv_w.shape), dconv_b.to(conv_b.dtype) if conv_b is not None else None,
                dbias_h.to(bias_dt), dA_h.to(A_dt), dD_h.to(D_dt), None if dnorm_w is None else dnorm_w.to(norm_w.dtype), None, None, None, None, None, None)


def spiral_ssd(zxbcdt, conv_w, conv_b, dt_bias, A, D, norm_w, eps, scan_index, scan_index_inv, d_inner, d_state):
    """Fused core of the Mamba-2 'spiral' mixer (see _SpiralSSDFn).  A = -exp(A_log) [H], dt_bias [H], D [H]."""
    with torch.autocast(device_type="cuda", enabled=False):
        return _SpiralSSDFn.apply(zxbcdt, conv_w, conv_b, dt_bias, A, D, norm_w, eps, scan_index, scan_index_inv, d_inner, d_state,
                                  torch.is_grad_enabled())


def mamba_split_conv1d_scan_combined(zxbcdt, conv1d_weight, conv1d_bias, dt_bias, A, D, chunk_size, initial_states=None,
                                     seq_idx=None, dt_limit=(0.0, float("inf")), return_final_states=False, activation="silu",
                                     rmsnorm_weight=None, rmsnorm_eps=1e-6, outproj_weight=None, outproj_bias=None, headdim=None,
                                     ngroups=1, norm_before_gate=True):
    """Drop-in for mamba_ssm's Mamba-2 fused operator with the keyword usage of block/mamba2.py:392-410.

    zxbcdt: (B, L, 2*dim + 2*ngroups*N + H), columns [z | x | B | C | dt].  Scalar D per head, ngroups 1.  Returns (B, L, d_model).
    The result does not depend on chunk_size: up to L = 224 the matrix-pipe kernels treat the sequence as one chunk, past that a
    no-grad call runs dm_ssd_fwd_chunked with the kernel's own chunk length (hip_ops.ssd_fwd_chunked), and every other call takes
    the A-shared scan, which has no chunks at all."""
    if initial_states is not None or seq_idx is not None or return_final_states or ngroups != 1 or headdim is None:
        raise NotImplementedError("only the call pattern of block/mamba2.py:392-410 is built (ngroups=1, scalar D, no states)")
    if activation not in ("silu", "swish") or dt_limit != (0.0, float("inf")):
        raise NotImplementedError("activation must be silu and dt_limit unbounded")
    Bsz, L, _ = zxbcdt.shape
    if rmsnorm_weight is not None and norm_before_gate:
        raise NotImplementedError("norm_before_gate=True (norm, then gate) is not wired; DiffMa uses norm_before_gate=False (block/mamba2.py:349)")
    H = D.shape[0]
    dim = H * headdim
    N = (zxbcdt.shape[-1] - 2 * dim - H) // 2
    if zxbcdt.stride(-1) != 1:
        zxbcdt = zxbcdt.contiguous()
    # ONE autograd node, the same one the Mamba2 module runs with three directions: conv (K3), the single-chunk SSD core on the
    # matrix pipe (dm_ssd_fwd / dm_ssd_bwd) when the shape allows it -- 16-bit I/O, headdim 64, 16-byte aligned rows, d_state 16 (or a
    # wide state of hip_ops.SSD_FWD_WIDTHS: without gradients, or with hip_ops.SSD_MFMA_BWD_WIDE on, dm_ssd_bwd_wide) --
    # past L = 224 without gradients the chunked forward (dm_ssd_fwd_chunked, hip_ops.SSD_FWD_CHUNKED_WIDTHS),
    # else the A-shared selective scan, then the gated RMSNorm (dm_rmsnorm_merge_*, one slab) when rmsnorm_weight is given.
    ident = _const("ident", L, zxbcdt.device)
    y = spiral_ssd(zxbcdt, conv1d_weight, conv1d_bias, dt_bias, A, D, rmsnorm_weight, rmsnorm_eps, ident, ident, dim, N)
    if outproj_weight is not None:
        y = F.linear(y, outproj_weight.to(y.dtype), outproj_bias)
    return y


def spiral_ssm(xz, conv_w, conv_b, x_proj_w, dt_proj_w, dt_proj_b, A, Dskip, scan_index, out_index=None, merge=True):
    """Fused CrossScan -> ndir x (conv1d+SiLU, x_proj, dt_proj, selective scan) -> CrossMerge (pre out_proj).

    xz: [B, L, 2*Din] token-major (the in_proj output); A: [Din, N] fp32 (= -exp(A_log));
    scan_index: int32 [ndir, L] device tensor (3 spiral directions for DiffMa; 1 / 2 / 4 for the baseline blocks).
    out_index / merge: see _SpiralSSMFn.forward.  Returns y [B, L, Din] (or [ndir, B, L, Din]); the caller applies out_proj.
    """
    with torch.autocast(device_type="cuda", enabled=False):
        return _SpiralSSMFn.apply(torch.is_grad_enabled(), out_index, merge, 1, None, xz, scan_index, conv_w, conv_b, x_proj_w, dt_proj_w,
                                  dt_proj_b.float(), A.float(), Dskip.float())[0]


# ------------------------------------------------------------------------------------------------
# The gate's backward inside out_proj's input gradient (csrc/gemm_large.hip, dm_gemm_large with gate_z set)
# ------------------------------------------------------------------------------------------------
# Backward of "merge output -> out_proj" at large batch: K12 forms dy = d(out) W tile by tile and the hoisted gate's backward reads
# it back at once (dm_gate_bwd: dy, z, pre -> g, dz).  With the gate applied in K12's epilogue dy never reaches memory (205 MB written
# and read per mixer at the bench batch, and one launch).  out_proj's weight gradient is d(out)^T y -- the gradient that ARRIVES and
# the saved merge output -- and out_proj has no bias here, so nothing else reads dy.  Taken when the gate is hoisted, the tensors are
# 16-bit and the input gradient would go to K12 as an NT product anyway; DIFFMA_GATE_IN_DGRAD=0 (hip_ops.GATE_IN_DGRAD) keeps the
# two launches.
class _GateDefer:
    """What the two autograd nodes of one mixer share: `taken` (set by _SpiralSSMFn.forward) and the d(xz) buffer, which
    _GatedOutProjFn.backward allocates (and writes the z half of) and _SpiralSSMFn.backward completes and returns -- one owner at a time."""
    __slots__ = ("taken", "dxz")

    def __init__(self):
        self.taken, self.dxz = False, None


def _gate_in_dgrad_rule(on_gpu, dtype, autocast_dtype, contiguous, wants_grad, xz_shape, w_shape):
    """The routing rule on plain values (so that it can be checked without a device): the switches; 16-bit activations that autocast
    would not change; a backward to come; and the shape test of projections.route for the input gradient dy [M, K = d_model] @ wt
    [N = d_inner, K]^T -- K12's shape rule (projections.large_shape), rows above the small-launch kernel's window, a shape K12 takes."""
    if not (hip_ops.GATE_IN_DGRAD and HOIST_GATE and proj.LARGE_DGRAD_NT and hip_ops.GEMM_LARGE):
        return False
    if not (on_gpu and len(xz_shape) == 3 and contiguous and wants_grad and dtype in (torch.bfloat16, torch.float16)):
        return False
    if autocast_dtype is not None and autocast_dtype != dtype:
        return False
    M, N, K = xz_shape[0] * xz_shape[1], w_shape[1], w_shape[0]
    if N * 2 != xz_shape[2] or not proj.large_shape(M, N, K) or proj.own_rows(SINGLE, M):
        return False
    code = {torch.bfloat16: _lib.DM_BF16, torch.float16: _lib.DM_F16}[dtype]
    return bool(_lib.load().dm_gemm_large_gated_supported(M, N, K, code))


def gate_in_dgrad_wanted(xz, weight):
    """Would out_proj's input gradient go to K12 as an NT product, with a hoisted gate in front of it?"""
    ac = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
    return _gate_in_dgrad_rule(xz.is_cuda, xz.dtype, ac, xz.is_contiguous(), torch.is_grad_enabled() and xz.requires_grad,
                               tuple(xz.shape), tuple(weight.shape))


class _GatedOutProjFn(torch.autograd.Function):
    """out = y W^T for the bias-free out_proj behind a mixer whose gate is hoisted (y = pre * silu(z), both from _SpiralSSMFn), with
    the gate's backward in the input gradient: the gradient returned for `pre` is g = (d(out) W) * silu(z), and dz is written into
    the z half of the d(xz) buffer that `defer` hands to _SpiralSSMFn.backward.  y is a value here, not a differentiable input."""

    @staticmethod
    def forward(ctx, y, pre, xz, weight, defer):
        wc = cast_weight(weight, y.dtype)
        ctx.save_for_backward(y, pre, xz, wc)
        ctx.defer, ctx.w_dt = defer, weight.dtype
        return product(FWD, SINGLE, y, wc)

    @staticmethod
    def backward(ctx, dout):
        y, pre, xz, wc = ctx.saved_tensors
        Bsz, L, D2 = xz.shape
        Din = D2 // 2
        with torch.autocast(device_type=y.device.type, enabled=False):
            dy2 = dout.reshape(-1, dout.shape[-1])
            if dy2.dtype != y.dtype:
                dy2 = dy2.to(y.dtype)
            dy2c = dy2.contiguous()
            dxz = torch.empty((1, Bsz, L, D2), dtype=xz.dtype, device=xz.device)
            z2, dz2, pre2 = xz.view(-1, D2)[:, Din:], dxz.view(-1, D2)[:, Din:], pre.view(-1, Din)
            wt = wc.t().contiguous()
            if hip_ops.gemm_large_gated_supported(dy2c, wt, z2, pre2, dz2):
                g = hip_ops.gemm_large_gated(dy2c, wt, z2, pre2, dz2).view(Bsz, L, Din)
            else:       # (a gradient layout that K12 does not take: the two launches, into the same buffers)
                dy = product(DGRAD, SINGLE, dy2c, wc, a_strided=dy2).view(Bsz, L, Din)
                g = hip_ops.gate_bwd(dy, xz[..., Din:], pre, dz_out=dxz[0][..., Din:])[0]
            dw = product(WGRAD, SINGLE, dy2c, y.reshape(-1, Din).contiguous()).to(ctx.w_dt) if ctx.needs_input_grad[3] else None
            ctx.defer.dxz = dxz
        return None, g, None, dw, None


def spiral_ssm_out_proj(xz, conv_w, conv_b, x_proj_w, dt_proj_w, dt_proj_b, A, Dskip, scan_index, out_proj_w):
    """linear_splitk(spiral_ssm(xz, ...), out_proj_w) for the bias-free out_proj of the spiral mixer where gate_in_dgrad_wanted says
    so: the gate's backward runs inside out_proj's input gradient (above)."""
    defer = _GateDefer()                 # (the caller asked gate_in_dgrad_wanted)
    with torch.autocast(device_type="cuda", enabled=False):
        outs = _SpiralSSMFn.apply(torch.is_grad_enabled(), None, True, 1, defer, xz, scan_index, conv_w, conv_b, x_proj_w, dt_proj_w,
                                  dt_proj_b.float(), A.float(), Dskip.float())
    if defer.taken:
        return _GatedOutProjFn.apply(outs[0], outs[1], xz, out_proj_w, defer)
    return linear_splitk(outs[0].to(xz.dtype), out_proj_w, None)


_CONSTS = {}


def _const(kind, n, device):
    """Identity row table / zero vector of the reference-facing operators, cached per (kind, size, device): the per-call
    torch.arange / torch.zeros were two launches of every mamba_inner_fn call (three calls per mixer on route A)."""
    key = (kind, int(n), str(device))
    t = _CONSTS.get(key)
    if t is None:
        # created OUTSIDE inference mode (an inference tensor cannot be saved for a later backward); not cached while a stream is
        # capturing (the tensor would live in that graph's private pool) -- ADVICE r4
        with torch.inference_mode(False):
            t = torch.arange(n, device=device, dtype=torch.int32)[None] if kind == "ident" else torch.zeros(n, device=device)
        if not (torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing()):
            _CONSTS[key] = t
    return t


def mamba_inner_fn(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight,
                   out_proj_bias, A, B=None, C=None, D=None, delta_bias=None, B_proj_bias=None,
                   C_proj_bias=None, delta_softplus=True):
    """Drop-in for mamba_ssm's mamba_inner_fn with the positional usage of block/mamba.py:346.

    xz: (B, 2*Din, L) (any strides; CrossScan hands out strided slices).  Returns (B, L, d_model).
    """
    if B is not None or C is not None or B_proj_bias is not None or C_proj_bias is not None:
        raise NotImplementedError("constant B/C and B/C projection biases are never used by DiffMa")
    if not delta_softplus:
        raise NotImplementedError("mamba_inner_fn is only defined with delta_softplus=True upstream")
    # [B, L, 2Din]: a view when xz is a transposed token-major buffer, one dm_repack pass when it is the reference's L-contiguous slice
    xzt = xz.transpose(1, 2) if xz.stride(1) == 1 else _RepackFn.apply(xz)
    ident = _const("ident", xzt.shape[1], xz.device)                              # made once per (length, device), not per call
    bias = delta_bias if delta_bias is not None else _const("zeros", xzt.shape[2] // 2, xz.device)
    Dsk = D if D is not None else _const("zeros", xzt.shape[2] // 2, xz.device)
    y = spiral_ssm(xzt, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, bias, A, Dsk, ident)
    # out_proj the way the native mixer runs it: K11 / K12 / the tuned library by size, the input gradient as an NT product, the
    # weight gradient split over the B L rows it contracts (F.linear's autograd hands those to untuned single-pass GEMMs)
    return linear_splitk(y, out_proj_weight, out_proj_bias)
