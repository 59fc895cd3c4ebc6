"""GPU parity of the individual HIP kernels (through the C ABI) against the CPU oracle.

Tolerances: fp32 I/O rtol 1e-4 / atol 1e-5 vs the fp64 recurrence; bf16 I/O 3e-2 / 5e-2;
fp16 3e-3 / 5e-3.  Integer work (row reindexing) is bit-exact.
"""
import math
import os
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.float32: (1e-4, 1e-5), torch.bfloat16: (3e-2, 5e-2), torch.float16: (3e-3, 5e-3)}


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def _inputs(S, L, Dm, N, dtype, seed, dev, with_z=True):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(S, L, Dm, generator=g)
    delta = torch.randn(S, L, Dm, generator=g) * 0.5
    z = torch.randn(S, L, Dm, generator=g) if with_z else None
    A = -(torch.rand(Dm, N, generator=g) * 4 + 0.2)
    Bm = torch.randn(S, L, N, generator=g)
    Cm = torch.randn(S, L, N, generator=g)
    Dp = torch.randn(Dm, generator=g)
    bias = torch.randn(Dm, generator=g) * 0.5
    cast = lambda t: None if t is None else t.to(dtype)
    host = dict(u=cast(u), delta=cast(delta), z=cast(z), A=A, B=cast(Bm), C=cast(Cm), D=Dp, bias=bias)
    devd = {k: (None if v is None else v.to(dev)) for k, v in host.items()}
    return host, devd


def _inputs_long_memory(S, L, Dm, N, dtype, seed, dev, with_z=True, a_shared=False):
    """_inputs where the state remembers, as the model initialises it (mamba.py / mamba2.py: A in [-16, -1], dt in [1e-3, 1e-1]):
    A[d, n] = -(n + 1) c_d with c_d log-uniform in [0.01, 1] (a_shared: A[d, :] = -16 c_d, one decay per channel), and a per-channel dt
    level log-uniform in [1e-3, 1e-1] times exp(0.3 randn) per step.  dt arrives as delta + bias BEFORE the softplus (bias = the
    level's pre-activation, delta the rest, rounded to the dtype), so the in-kernel softplus is still what runs.  A slow channel keeps
    e^(-0.01 * 1e-3 * 196) of state 0 over 196 steps; _inputs keeps e^-200."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(S, L, Dm, generator=g)
    z = torch.randn(S, L, Dm, generator=g) if with_z else None
    c = torch.exp(torch.rand(Dm, generator=g) * math.log(100.0)) * 0.01
    A = -16.0 * c[:, None].expand(Dm, N).contiguous() if a_shared else -(torch.arange(N) + 1.0)[None, :] * c[:, None]
    level = torch.exp(torch.rand(Dm, generator=g) * math.log(100.0)) * 1e-3
    dt = level * torch.exp(0.3 * torch.randn(S, L, Dm, generator=g))
    inv = lambda t: torch.log(torch.expm1(t.double())).float()                  # softplus^-1
    bias = inv(level)
    delta = inv(dt) - bias
    Bm = torch.randn(S, L, N, generator=g)
    Cm = torch.randn(S, L, N, generator=g)
    Dp = torch.randn(Dm, generator=g)
    cast = lambda t: None if t is None else t.to(dtype)
    host = dict(u=cast(u), delta=cast(delta), z=cast(z), A=A, B=cast(Bm), C=cast(Cm), D=Dp, bias=bias)
    devd = {k: (None if v is None else v.to(dev)) for k, v in host.items()}
    return host, devd


def _oracle_scan(h, softplus=True):
    from oracle.mamba_ref import selective_scan_ref

    cm = lambda t: None if t is None else t.float().permute(0, 2, 1).double()
    y, last = selective_scan_ref(cm(h["u"]), cm(h["delta"]), h["A"].double(), cm(h["B"]), cm(h["C"]),
                                 h["D"].double(), z=cm(h["z"]), delta_bias=h["bias"].double(),
                                 delta_softplus=softplus, return_last_state=True)
    return y.permute(0, 2, 1), last  # [S, L, D], [S, D, N]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("S,L,Dm", [(2, 196, 1024), (3, 49, 128), (2, 16, 64), (1, 7, 200), (2, 1, 64)])
def test_scan_fwd_matches_oracle(gpu, dtype, S, L, Dm):
    from diffma_amd import hip_ops

    N = 16
    host, d = _inputs(S, L, Dm, N, dtype, seed=L * 7 + Dm, dev=gpu)
    last = torch.empty(S, N, Dm, device=gpu)
    out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["bias"], True,
                           last_state=last)
    torch.cuda.synchronize()
    ref, ref_last = _oracle_scan(host)
    rtol, atol = TOL[dtype]
    torch.testing.assert_close(out.float().cpu().double(), ref, rtol=rtol, atol=atol * max(1.0, ref.abs().max().item()))
    torch.testing.assert_close(last.cpu().double().permute(0, 2, 1), ref_last, rtol=1e-4, atol=1e-5 * max(1.0, ref_last.abs().max().item()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L,Dm,with_z", [(196, 128, True), (100, 200, True), (57, 64, False), (183, 128, True)])
def test_scan_fwd_chunk_parallel_variant(gpu, dtype, L, Dm, with_z):
    """Small launches without checkpoints take the chunk-parallel kernel (csrc/scan_fwd_chunked.h: 14 waves x 14 steps,
    two passes); ragged L / dim, row-index gather + scatter with 3 directions sharing one z."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import selective_scan_ref

    Bsz, ndir, N = 2, 3, 16
    S = Bsz * ndir
    host, d = _inputs(S, L, Dm, N, dtype, seed=L + Dm, dev=gpu, with_z=False)
    g = torch.Generator().manual_seed(9)
    zsrc = torch.randn(Bsz, L, Dm, generator=g).to(dtype) if with_z else None
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    operms = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)]).int()
    ckpt = None
    if with_z:
        if dtype == torch.float32:                   # training form of the same launch: checkpoints every 4 steps from pass 2
            ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dtype, gpu).zero_()
        out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], zsrc.to(gpu), d["bias"], True,
                               z_row_index=perms.to(gpu), out_row_index=operms.to(gpu), batch_per_dir=Bsz, ckpt=ckpt)
    else:
        out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], None, d["bias"], True)
    torch.cuda.synchronize()
    out = out.float().cpu()
    rtol, atol = TOL[dtype]
    for s in range(S):
        k, b = divmod(s, Bsz)
        cm = lambda t: t[s:s + 1].float().permute(0, 2, 1).double()
        zz = zsrc[b][perms[k].long()].float().T[None].double() if with_z else None
        ref = selective_scan_ref(cm(host["u"]), cm(host["delta"]), host["A"].double(), cm(host["B"]), cm(host["C"]),
                                 host["D"].double(), z=zz, delta_bias=host["bias"].double(), delta_softplus=True)[0].T
        got = out[s][operms[k].long()] if with_z else out[s]
        torch.testing.assert_close(got.double(), ref, rtol=rtol, atol=atol * max(1.0, ref.abs().max().item()))
        if ckpt is not None and s in (0, S - 1):
            K = hip_ops.SCAN_CKPT_EVERY
            for c in (0, 1, 3, 4, (L - 1) // K):     # incl. boundaries that fall inside and between the 14-step wave chunks; slot 0 = final state
                n = c * K if c else L
                _, hl = selective_scan_ref(cm(host["u"])[..., :n], cm(host["delta"])[..., :n], host["A"].double(),
                                           cm(host["B"])[..., :n], cm(host["C"])[..., :n], None, z=None,
                                           delta_bias=host["bias"].double(), delta_softplus=True, return_last_state=True)
                torch.testing.assert_close(ckpt[s, c].cpu().double().T, hl[0], rtol=1e-4, atol=1e-5 * max(1.0, hl.abs().max().item()))


def _ckpt_states(ckpt, N, Dm):
    """The checkpoint buffer as fp32 states [S, chunk, N, Dm]: fp32 as stored; the packed bf16 form [S, chunk, N/8 * Dm, 4] int32 holds
    word w of (group g, channel d) = states 8 g + 2 w (low half) and 8 g + 2 w + 1 (high half) (csrc/scan_fwd_impl.h store_slot)."""
    if ckpt.dtype != torch.int32:
        return ckpt.float()
    S, nck = ckpt.shape[:2]
    w = ckpt.view(S, nck, N // 8, Dm, 4)
    lo, hi = (w << 16).view(torch.float32), (w & -65536).view(torch.float32)
    return torch.stack([lo, hi], -1).permute(0, 1, 2, 4, 5, 3).reshape(S, nck, N, Dm)


def _oracle_states(host, s):
    """fp64 state after every step of sequence s, [L, Dm, N]: h_l = exp(dt_l A) h_{l-1} + dt_l u_l B_l, dt = softplus(delta + bias)."""
    from oracle.mamba_ref import softplus_ref

    d64 = lambda t: t[s].float().double()
    dt = softplus_ref(d64(host["delta"]) + host["bias"].double())
    dA = torch.exp(dt[:, :, None] * host["A"].double()[None])
    dBu = (dt * d64(host["u"]))[:, :, None] * d64(host["B"])[:, None, :]
    h, hs = torch.zeros_like(dA[0]), []
    for l in range(dt.shape[0]):
        h = dA[l] * h + dBu[l]
        hs.append(h)
    return torch.stack(hs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("L", [196, 183])
def test_scan_fwd_chunk_parallel_long_memory(gpu, dtype, L):
    """The chunk-parallel forward with checkpoints on _inputs_long_memory, where the carry folded across the 14 wave chunks is O(1)
    instead of 1e-10: outputs at the tolerances of the file, and EVERY checkpoint slot (49 at L = 196: the state entering every
    4-step sub-chunk, so all 14 chunk entries and every slot between them; slot 0 = the final state) of the first and the last
    sequence against the fp64 state.  fp32 checkpoints (fp32 and fp16 I/O): rtol 1e-4 / atol 1e-5 max|h| as in the tests above.
    Packed bf16 checkpoints: the kernel rounds its fp32 state once (v_cvt_pk_bf16_f32), so u |h| + (1 + u) x that fp32 tolerance,
    u = 2^-8 -- the oracle state rounded to the format, give or take the fp32 error that can move it across a rounding boundary."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import selective_scan_ref

    Bsz, ndir, N, Dm = 2, 3, 16, 128
    S = Bsz * ndir
    host, d = _inputs_long_memory(S, L, Dm, N, dtype, seed=L + Dm, dev=gpu, with_z=False)
    g = torch.Generator().manual_seed(9)
    zsrc = torch.randn(Bsz, L, Dm, generator=g).to(dtype)
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    operms = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)]).int()
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dtype, gpu).zero_()
    out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], zsrc.to(gpu), d["bias"], True, z_row_index=perms.to(gpu),
                           out_row_index=operms.to(gpu), batch_per_dir=Bsz, ckpt=ckpt, variant="chunked")
    torch.cuda.synchronize()
    out = out.float().cpu()
    got_h = _ckpt_states(ckpt, N, Dm).cpu().double()
    rtol, atol = TOL[dtype]
    K = hip_ops.SCAN_CKPT_EVERY
    for s in range(S):
        k, b = divmod(s, Bsz)
        cm = lambda t: t[s:s + 1].float().permute(0, 2, 1).double()
        zz = zsrc[b][perms[k].long()].float().T[None].double()
        ref, last = selective_scan_ref(cm(host["u"]), cm(host["delta"]), host["A"].double(), cm(host["B"]), cm(host["C"]), host["D"].double(),
                                       z=zz, delta_bias=host["bias"].double(), delta_softplus=True, return_last_state=True)
        torch.testing.assert_close(out[s][operms[k].long()].double(), ref[0].T, rtol=rtol, atol=atol * max(1.0, ref.abs().max().item()))
        if s in (0, S - 1):
            hs = _oracle_states(host, s)
            assert float((hs[-1] - last[0]).abs().max()) <= 1e-12 * float(last.abs().max())          # the restatement is the oracle's
            for c in range(hip_ops.scan_nchunk(L, K)):
                want = hs[(c * K if c else L) - 1].T                                                    # [N, Dm]
                tol32 = 1e-4 * want.abs() + 1e-5 * max(1.0, float(want.abs().max()))
                tol = tol32 if ckpt.dtype != torch.int32 else 2.0 ** -8 * want.abs() + (1 + 2.0 ** -8) * tol32
                err = (got_h[s, c] - want).abs()
                assert bool((err <= tol).all()), (s, c, float((err / tol).max()))


@pytest.mark.parametrize("softplus,with_z", [(False, True), (True, False), (False, False)])
def test_scan_fwd_flags(gpu, softplus, with_z):
    from diffma_amd import hip_ops
    from oracle.mamba_ref import selective_scan_ref

    S, L, Dm, N = 2, 33, 128, 16
    host, d = _inputs(S, L, Dm, N, torch.float32, seed=5, dev=gpu, with_z=with_z)
    if not softplus:  # raw deltas must be positive-ish to keep the recurrence bounded
        host["delta"] = host["delta"].abs() * 0.3
        d["delta"] = host["delta"].to(gpu)
    out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], None, d["z"], None, softplus)
    cm = lambda t: None if t is None else t.permute(0, 2, 1).double()
    ref = selective_scan_ref(cm(host["u"]), cm(host["delta"]), host["A"].double(), cm(host["B"]), cm(host["C"]),
                             None, z=cm(host["z"]), delta_bias=None, delta_softplus=softplus).permute(0, 2, 1)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-4, atol=1e-5 * max(1.0, ref.abs().max().item()))


def test_scan_fwd_row_index_and_checkpoints(gpu):
    """z gathered through z_row_index, output scattered through out_row_index, ndir=3 sharing one z;
    checkpoints equal the oracle's running state at the chunk boundaries."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import selective_scan_ref

    Bsz, ndir, L, Dm, N = 2, 3, 40, 128, 16
    S = Bsz * ndir
    host, d = _inputs(S, L, Dm, N, torch.float32, seed=11, dev=gpu)
    g = torch.Generator().manual_seed(3)
    zsrc = torch.randn(Bsz, L, Dm, generator=g)
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    operms = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)]).int()
    K = hip_ops.SCAN_CKPT_EVERY
    nch = hip_ops.scan_nchunk(L, K)
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, torch.float32, gpu).zero_()
    out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], zsrc.to(gpu), d["bias"], True,
                           z_row_index=perms.to(gpu), out_row_index=operms.to(gpu), batch_per_dir=Bsz,
                           ckpt=ckpt, ckpt_every=K)
    torch.cuda.synchronize()
    out = out.cpu()
    for s in range(S):
        k, b = divmod(s, Bsz)
        zz = zsrc[b][perms[k].long()]  # [L, Dm]
        cm = lambda t: t[s:s + 1].permute(0, 2, 1).double()
        ref = selective_scan_ref(cm(host["u"]), cm(host["delta"]), host["A"].double(), cm(host["B"]), cm(host["C"]),
                                 host["D"].double(), z=zz.T[None].double(), delta_bias=host["bias"].double(),
                                 delta_softplus=True)[0].T  # [L, Dm] in scan order
        got = out[s][operms[k].long()]  # row operm[l] holds step l
        torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-5 * max(1.0, ref.abs().max().item()))
        for c in range(0, nch):                    # slot 0 = the state after the last step, slot c > 0 = state entering step c*K
            n = c * K if c else L
            _, hl = selective_scan_ref(cm(host["u"])[..., :n], cm(host["delta"])[..., :n], host["A"].double(),
                                       cm(host["B"])[..., :n], cm(host["C"])[..., :n], None, z=None,
                                       delta_bias=host["bias"].double(), delta_softplus=True, return_last_state=True)
            torch.testing.assert_close(ckpt[s, c].cpu().double().T, hl[0], rtol=1e-4, atol=1e-5 * max(1.0, hl.abs().max().item()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L,Dm,ndir,with_ckpt", [(2, 196, 256, 3, True), (3, 49, 128, 3, False), (2, 37, 200, 4, True), (1, 13, 64, 2, False)])
def test_scan_fwd_accumulates_directions(gpu, dtype, Bsz, L, Dm, ndir, with_ckpt):
    """DM_FLAG_ACC_DIRS: one wave walks the ndir directions of a batch element and accumulates them into ONE token-order buffer
    (CrossMerge folded into the scan) -- against the oracle scan per direction scattered and summed in fp64, and the
    checkpoints of every direction still equal the unmerged launch's."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import selective_scan_ref

    N = 16
    S = Bsz * ndir
    host, d = _inputs(S, L, Dm, N, dtype, seed=L + Dm + ndir, dev=gpu, with_z=False)
    g = torch.Generator().manual_seed(5)
    zsrc = torch.randn(Bsz, L, Dm, generator=g).to(dtype)
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    operms = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)]).int()
    ck1 = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dtype, gpu).zero_() if with_ckpt else None
    ck2 = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dtype, gpu).zero_() if with_ckpt else None
    kw = dict(z_row_index=perms.to(gpu), out_row_index=operms.to(gpu), batch_per_dir=Bsz)
    merged = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], zsrc.to(gpu), d["bias"], True, ckpt=ck1, acc_dirs=True, **kw)
    plain = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], zsrc.to(gpu), d["bias"], True, ckpt=ck2,
                             variant="sequential", **kw)
    torch.cuda.synchronize()
    assert merged.shape == (Bsz, L, Dm)
    if with_ckpt:
        assert torch.equal(ck1, ck2)
    ref = torch.zeros(Bsz, L, Dm, dtype=torch.float64)
    for s_ in range(S):
        k, b = divmod(s_, Bsz)
        cm = lambda t: t[s_:s_ + 1].float().permute(0, 2, 1).double()
        zz = zsrc[b][perms[k].long()].float().T[None].double()
        y = selective_scan_ref(cm(host["u"]), cm(host["delta"]), host["A"].double(), cm(host["B"]), cm(host["C"]),
                               host["D"].double(), z=zz, delta_bias=host["bias"].double(), delta_softplus=True)[0].T      # [L, Dm] scan order
        ref[b] = ref[b].index_add(0, operms[k].long(), y)
    rtol, atol = TOL[dtype]
    torch.testing.assert_close(merged.float().cpu().double(), ref, rtol=rtol, atol=atol * ndir * max(1.0, ref.abs().max().item()))
    # and against the separate merge pass over the unmerged launch (same values up to the rounding of the running sum)
    tm = hip_ops.token_merge(plain.view(ndir, Bsz, L, Dm))
    torch.testing.assert_close(merged.float(), tm.float(), rtol=rtol, atol=atol * max(1.0, ref.abs().max().item()))


@pytest.mark.parametrize("N", [8, 32, 64])
def test_scan_fwd_other_dstate(gpu, N):
    from diffma_amd import hip_ops

    S, L, Dm = 2, 21, 64
    host, d = _inputs(S, L, Dm, N, torch.float32, seed=N, dev=gpu)
    out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["bias"], True)
    ref, _ = _oracle_scan(host)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-4, atol=1e-5 * max(1.0, ref.abs().max().item()))


def test_scan_linearity_in_u_full_size(gpu):
    """Size-independent property at the bench shape: for fixed delta/B/C the operator is linear in u
    (y(u1+u2) = y(u1)+y(u2) when D-skip and z gate act multiplicatively on the same z)."""
    from diffma_amd import hip_ops

    S, L, Dm, N = 96, 196, 1024, 16
    g = torch.Generator(device="cpu").manual_seed(0)
    mk = lambda *s: torch.randn(*s, generator=g).to(gpu)
    u1, u2, delta, z = mk(S, L, Dm), mk(S, L, Dm), mk(S, L, Dm) * 0.5, mk(S, L, Dm)
    A = -(torch.rand(Dm, N, generator=g) * 4 + 0.2).to(gpu)
    Bm, Cm, Dp, bias = mk(S, L, N), mk(S, L, N), mk(Dm), mk(Dm) * 0.5
    f = lambda u: hip_ops.scan_fwd(u, delta, A, Bm, Cm, Dp, z, bias, True)
    y12, y1, y2 = f(u1 + u2), f(u1), f(u2)
    scale = y12.abs().max().item()
    assert torch.isfinite(y12).all()
    torch.testing.assert_close(y12, y1 + y2, rtol=1e-4, atol=2e-5 * scale)


def test_scan_bwd_linearity_in_dout_full_size(gpu):
    """Size-independent property of the adjoint at the bench's channel count: every gradient is linear in dout,
    and the input gradients agree with the forward through <dout, J du> = <J^T dout, du> (dot-product test in u)."""
    from diffma_amd import hip_ops

    S, L, Dm, N = 48, 196, 1024, 16
    g = torch.Generator(device="cpu").manual_seed(1)
    mk = lambda *s: torch.randn(*s, generator=g).to(gpu)
    u, delta, z = mk(S, L, Dm), mk(S, L, Dm) * 0.5, mk(S, L, Dm)
    A = -(torch.rand(Dm, N, generator=g) * 4 + 0.2).to(gpu)
    Bm, Cm, Dp, bias = mk(S, L, N), mk(S, L, N), mk(Dm), mk(Dm) * 0.5
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, torch.float32, gpu)
    f = lambda uu: hip_ops.scan_fwd(uu, delta, A, Bm, Cm, Dp, z, bias, True, ckpt=ckpt)
    f(u)
    bwd = lambda d: hip_ops.scan_bwd(u, delta, A, Bm, Cm, Dp, z, bias, d, ckpt, True)
    d1, d2 = mk(S, L, Dm), mk(S, L, Dm)
    r12, r1, r2 = bwd(d1 + d2), bwd(d1), bwd(d2)
    for name, a, b, c in zip(("du", "ddelta", "dz", "dB", "dC", "dA", "dD", "dbias"), r12, r1, r2):
        scale = max(a.abs().max().item(), 1e-6)
        assert torch.isfinite(a).all(), name
        torch.testing.assert_close(a, b + c, rtol=2e-4, atol=3e-5 * scale, msg=lambda m, n=name: f"{n}: {m}")
    # dot-product test: the operator is linear in u, so <d1, f(v) - f(0)> == <J_u^T d1, v> for any v
    v = mk(S, L, Dm)
    lhs = (d1.double() * (f(v).double() - f(torch.zeros_like(v)).double())).sum()
    f(u)                                                        # restore the checkpoints of the point bwd was taken at
    rhs = (r1[0].double() * v.double()).sum()
    assert abs(lhs - rhs) <= 2e-4 * max(abs(lhs), abs(rhs), 1.0), (float(lhs), float(rhs))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Bsz,L,Dm,W", [(2, 196, 1024, 4), (3, 49, 128, 4), (1, 16, 64, 3), (2, 5, 200, 2), (1, 1, 64, 4)])
def test_gather_conv_fwd_matches_oracle(gpu, dtype, Bsz, L, Dm, W):
    from diffma_amd import hip_ops
    from oracle.mamba_ref import causal_conv1d_ref

    g = torch.Generator().manual_seed(L + Dm)
    xz = torch.randn(Bsz, L, 2 * Dm, generator=g).to(dtype)
    w = torch.randn(Dm, W, generator=g) * 0.5
    b = torch.randn(Dm, generator=g) * 0.1
    ndir = 3
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    out = hip_ops.gather_conv1d_fwd(xz.to(gpu)[..., :Dm], w.to(gpu), b.to(gpu), row_index=perms.to(gpu), ndir=ndir)
    out = out.float().cpu().view(ndir, Bsz, L, Dm)
    rtol, atol = TOL[dtype]
    for k in range(ndir):
        xs = xz[..., :Dm].float()[:, perms[k].long(), :]                    # gathered tokens [B, L, Dm]
        ref = causal_conv1d_ref(xs.permute(0, 2, 1).double(), w.double(), b.double(), activation="silu").permute(0, 2, 1)
        torch.testing.assert_close(out[k].double(), ref, rtol=rtol, atol=atol)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L,Dm,P,W,with_idx", [(2, 196, 1024, 64, 4, True), (3, 49, 128, 36, 4, True), (1, 16, 128, 40, 4, False),
                                                   (2, 37, 256, 64, 3, True), (1, 1, 512, 16, 2, False), (2, 5, 1024, 33, 4, True)])
def test_fused_conv_xproj_fwd_matches_oracle(gpu, dtype, Bsz, L, Dm, P, W, with_idx):
    """K3x (csrc/conv_xproj.hip): x~ = SiLU(conv(gathered x)) and x_dbl = x~ @ Wx^T from one kernel vs the fp64 oracle conv and an
    fp64 product of the ROUNDED x~ (that is what mamba_inner_fn's x_proj sees as well).  Ragged L (partial last tile), projection
    widths that are not a multiple of 16, all conv widths, with and without the 3-direction gather."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import causal_conv1d_ref

    g = torch.Generator().manual_seed(L * 3 + Dm + P)
    xz = torch.randn(Bsz, L, 2 * Dm, generator=g).to(dtype)
    w = torch.randn(Dm, W, generator=g) * 0.5
    b = torch.randn(Dm, generator=g) * 0.1
    wx = (torch.randn(P, Dm, generator=g) * 0.1).to(dtype)
    ndir = 3 if with_idx else 1
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    xc, xdbl = hip_ops.gather_conv1d_xproj_fwd(xz.to(gpu)[..., :Dm], w.to(gpu), b.to(gpu), wx.to(gpu),
                                               row_index=perms.to(gpu) if with_idx else None, ndir=ndir)
    torch.cuda.synchronize()
    assert xc.shape == (ndir * Bsz, L, Dm) and xdbl.shape == (ndir * Bsz * L, P)
    xc_c = xc.float().cpu().view(ndir, Bsz, L, Dm)
    rtol, atol = TOL[dtype]
    for k in range(ndir):
        xs = xz[..., :Dm].float()[:, perms[k].long(), :]
        ref = causal_conv1d_ref(xs.permute(0, 2, 1).double(), w.double(), b.double(), activation="silu").permute(0, 2, 1)
        torch.testing.assert_close(xc_c[k].double(), ref, rtol=rtol, atol=atol)
    # the same x~ as the unfused conv kernel: identical arithmetic, so at most a rounding tie resolved the other way (fp32
    # contraction is the compiler's choice per kernel) -- never more than one 16-bit ulp, on a vanishing fraction of elements
    plain = hip_ops.gather_conv1d_fwd(xz.to(gpu)[..., :Dm], w.to(gpu), b.to(gpu), row_index=perms.to(gpu) if with_idx else None, ndir=ndir)
    diff = (plain.float() - xc.float()).abs()
    assert float((diff > 0).float().mean()) <= 1e-4
    assert bool((diff <= plain.float().abs() * 2.0 ** (-7 if dtype == torch.bfloat16 else -10) + 1e-30).all())
    ref_dbl = xc.float().cpu().double().view(-1, Dm) @ wx.float().double().t()
    torch.testing.assert_close(xdbl.float().cpu().double(), ref_dbl, rtol=rtol, atol=atol * max(1.0, ref_dbl.abs().max().item()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L,Dm,P,W,with_idx", [(2, 196, 1024, 64, 4, True), (3, 49, 128, 64, 4, True), (1, 16, 128, 64, 4, False),
                                                   (2, 37, 256, 64, 3, True), (1, 1, 512, 64, 2, False), (2, 5, 1024, 64, 4, True)])
def test_fused_conv_xproj_bwd_matches_oracle_autograd(gpu, dtype, Bsz, L, Dm, P, W, with_idx):
    """K4x: conv backward with the incoming gradient du + dx_dbl @ Wx formed in the kernel, against fp64 autograd of
    loss = <du, x~> + <dx_dbl, x~ @ Wx^T> through the oracle conv: dx per direction (token order), dweight, dbias."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import causal_conv1d_ref

    g = torch.Generator().manual_seed(L * 5 + Dm + P)
    xz = torch.randn(Bsz, L, 2 * Dm, generator=g).to(dtype)
    w = torch.randn(Dm, W, generator=g) * 0.5
    b = torch.randn(Dm, generator=g) * 0.1
    wx = (torch.randn(P, Dm, generator=g) * 0.1).to(dtype)
    ndir = 3 if with_idx else 1
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    du = torch.randn(ndir * Bsz, L, Dm, generator=g).to(dtype)
    dxdbl = torch.randn(ndir * Bsz * L, P, generator=g).to(dtype)
    dx, dw, db = hip_ops.gather_conv1d_xproj_bwd(xz.to(gpu)[..., :Dm], w.to(gpu), b.to(gpu), du.to(gpu), dxdbl.to(gpu),
                                                 wx.to(gpu).t().contiguous(), row_index=perms.to(gpu) if with_idx else None, ndir=ndir)
    torch.cuda.synchronize()
    x = xz[..., :Dm].float().double().clone().requires_grad_(True)
    wd, bd = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    wx64 = wx.float().double()
    loss, per_dir = 0, []
    for k in range(ndir):
        xs = x[:, perms[k].long(), :]
        y = causal_conv1d_ref(xs.permute(0, 2, 1), wd, bd, activation="silu").permute(0, 2, 1)          # [B, L, Dm]
        lk = (y * du.view(ndir, Bsz, L, Dm)[k].float().double()).sum() + ((y.reshape(-1, Dm) @ wx64.t()) * dxdbl.view(ndir, Bsz * L, P)[k].float().double()).sum()
        per_dir.append(torch.autograd.grad(lk, x, retain_graph=True)[0])
        loss = loss + lk
    loss.backward()
    rtol, atol = {torch.bfloat16: (3e-2, 5e-2), torch.float16: (4e-3, 8e-3)}[dtype]
    got = dx.float().cpu().double().view(ndir, Bsz, L, Dm)
    for k in range(ndir):
        sc = max(1.0, per_dir[k].abs().max().item())
        torch.testing.assert_close(got[k], per_dir[k], rtol=rtol, atol=atol * sc, msg=lambda m, k=k: f"dx dir {k}: {m}")
    sc = max(1.0, wd.grad.abs().max().item())
    torch.testing.assert_close(dw.cpu().double(), wd.grad, rtol=rtol, atol=atol * sc * 0.2)
    torch.testing.assert_close(db.cpu().double(), bd.grad, rtol=rtol, atol=atol * sc * 0.2)


def test_token_merge_exact(gpu):
    from diffma_amd import hip_ops

    K, Bsz, L, Dm = 3, 2, 49, 128
    g = torch.Generator().manual_seed(1)
    slabs = torch.randn(K, Bsz, L, Dm, generator=g)
    idx = torch.stack([torch.randperm(L, generator=g) for _ in range(K)]).int()
    out = hip_ops.token_merge(slabs.to(gpu), row_index=idx.to(gpu)).cpu()
    ref = sum(slabs[k][:, idx[k].long(), :] for k in range(K))
    # same summation order (k = 0,1,2) in fp32 => bit-exact
    assert torch.equal(out, (slabs[0][:, idx[0].long()] + slabs[1][:, idx[1].long()]) + slabs[2][:, idx[2].long()])
    torch.testing.assert_close(out, ref)
    out2 = hip_ops.token_merge(slabs.to(gpu)).cpu()
    assert torch.equal(out2, (slabs[0] + slabs[1]) + slabs[2])


def _oracle_device(gpu, elems):
    """Where the oracle's torch code (fp64 autograd through oracle/mamba_ref.py) runs for one test case: the host for small cases,
    the DEVICE for the full-width ones -- the same oracle functions on ATen's fp64 kernels instead of 30-60 s of host time per case
    (the GPU suite has a 1 200 s limit; DIFFMA_TEST_ORACLE_ON_HOST=1 puts everything back on the host)."""
    if os.environ.get("DIFFMA_TEST_ORACLE_ON_HOST") == "1" or elems < (1 << 18):
        return torch.device("cpu")
    return gpu


def _grads_to_cpu(*leaves):
    """Leaves of an oracle autograd run -> stand-ins that carry `.grad` on the host (the checks compare on the host)."""
    import types
    return [None if t is None else types.SimpleNamespace(grad=None if t.grad is None else t.grad.detach().cpu()) for t in leaves]


def _scan_bwd_case(gpu, dtype, S, L, Dm, N, seed, with_z=True, indexed=False, Bsz=None, a_shared=False, dout_per_seq=False,
                   variant="sequential", long_memory=False, delta_softplus=True, bc_fp32=False):
    """delta_softplus=False: delta + bias is used as it is (the kernels' delta mode 0), so both are made positive here; bc_fp32: B / C
    travel as fp32 tensors (holding the values rounded to dtype) next to 16-bit u / delta / z / dout.  a_shared: A[d, :] is one value per channel and the kernels run their DM_FLAG_A_SHARED form (one exp per channel-step, the
    Mamba-2 call pattern); dout_per_seq: the incoming gradient is per direction [S, L, Dm] in token order, read through
    out_row_index (DM_FLAG_DOUT_PER_SEQ) instead of one merged gradient per batch element."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import selective_scan_ref

    if long_memory:
        host, d = _inputs_long_memory(S, L, Dm, N, dtype, seed=seed, dev=gpu, with_z=with_z and not indexed, a_shared=a_shared)
    else:
        host, d = _inputs(S, L, Dm, N, dtype, seed=seed, dev=gpu, with_z=with_z and not indexed)
    if a_shared:
        host["A"] = host["A"][:, :1].expand(Dm, N).contiguous()
        d["A"] = host["A"].to(gpu)
    if not delta_softplus:                 # a negative step would make the state grow: activate delta here, keep a small positive bias
        host["delta"] = torch.nn.functional.softplus(host["delta"].float() + host["bias"]).to(dtype)
        host["bias"] = host["bias"].abs() * 0.1
        d["delta"], d["bias"] = host["delta"].to(gpu), host["bias"].to(gpu)
    if bc_fp32:
        d["B"], d["C"] = host["B"].float().to(gpu), host["C"].float().to(gpu)
    g = torch.Generator().manual_seed(seed + 1)
    K = hip_ops.SCAN_CKPT_EVERY
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dtype, gpu).zero_()
    kw = {}
    if indexed:
        ndir = S // Bsz
        zsrc = torch.randn(Bsz, L, Dm, generator=g).to(dtype) if with_z else None       # no gate: the tables still route dout / out
        zperm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)]).int()
        operm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)]).int()
        kw = dict(z_row_index=zperm.to(gpu), out_row_index=operm.to(gpu), batch_per_dir=Bsz)
        zdev = None if zsrc is None else zsrc.to(gpu)
        # gradient of the MERGED output (token order), or one gradient per direction (token order as well)
        dout = torch.randn(S if dout_per_seq else Bsz, L, Dm, generator=g).to(dtype)
    else:
        zdev = d["z"]
        dout = torch.randn(S, L, Dm, generator=g).to(dtype)
    # variant: the kernel family under test (both the forward that writes the checkpoints and the backward); the library's own
    # choice by launch size would send every small test shape to the chunk-parallel kernels
    fwd_variant = variant if (variant != "chunked" or (16 * 14 // 4 < L <= 196 and N == 16)) else "sequential"
    out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], zdev, d["bias"], delta_softplus,
                           ckpt=ckpt, ckpt_every=K, a_shared=a_shared, variant=fwd_variant, **kw)
    res = hip_ops.scan_bwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], zdev, d["bias"], dout.to(gpu), ckpt,
                           delta_softplus, ckpt_every=K, a_shared=a_shared, dout_per_seq=dout_per_seq, variant=variant, **kw)
    torch.cuda.synchronize()
    du, ddelta, dz, dB, dC, dA, dD, dbias = [None if t is None else t.float().cpu().double() for t in res]

    # fp64 autograd of the oracle on the same (rounded) inputs; the big cases run the oracle's torch code on the device (_oracle_device)
    odev = _oracle_device(gpu, S * L * Dm)
    leaf = lambda t: t.float().double().to(odev).clone().requires_grad_(True)
    u, dl, A, Bm, Cm, Dp, bias = leaf(host["u"]), leaf(host["delta"]), leaf(host["A"]), leaf(host["B"]), leaf(host["C"]), leaf(host["D"]), leaf(host["bias"])
    cm = lambda t: t.permute(0, 2, 1)
    dout_o = dout.float().double().to(odev)
    if indexed:
        z = leaf(zsrc) if with_z else None
        ndir = S // Bsz
        zp_o, op_o = zperm.long().to(odev), operm.long().to(odev)
        zs = None if z is None else torch.cat([z[:, zp_o[k], :] for k in range(ndir)], 0)        # [S, L, Dm] gathered
        y = cm(selective_scan_ref(cm(u), cm(dl), A, cm(Bm), cm(Cm), Dp, z=None if zs is None else cm(zs), delta_bias=bias,
                                  delta_softplus=delta_softplus))
        # scatter: merged[b, operm[k][l]] += y[k*Bsz+b, l]
        if dout_per_seq:                   # direction k's step l lands in row operm[k][l] of ITS OWN token-order slab
            loss = 0
            for k in range(ndir):
                slab = torch.zeros(Bsz, L, Dm, dtype=torch.float64, device=odev).index_add(1, op_o[k], y[k * Bsz:(k + 1) * Bsz])
                loss = loss + (slab * dout_o[k * Bsz:(k + 1) * Bsz]).sum()
        else:
            merged = torch.zeros(Bsz, L, Dm, dtype=torch.float64, device=odev)
            for k in range(ndir):
                merged = merged.index_add(1, op_o[k], y[k * Bsz:(k + 1) * Bsz])
            loss = (merged * dout_o).sum()
    else:
        z = leaf(host["z"]) if with_z else None
        y = cm(selective_scan_ref(cm(u), cm(dl), A, cm(Bm), cm(Cm), Dp, z=None if z is None else cm(z), delta_bias=bias,
                                  delta_softplus=delta_softplus))
        loss = (y * dout_o).sum()
    loss.backward()
    u, dl, A, Bm, Cm, Dp, bias, z = _grads_to_cpu(u, dl, A, Bm, Cm, Dp, bias, z)
    y = y.detach().cpu()
    rtol, atol = {torch.float32: (2e-4, 2e-5), torch.bfloat16: (4e-2, 6e-2), torch.float16: (5e-3, 8e-3)}[dtype]
    # the forward of the same launch (gated output) against the oracle too
    rf, af = TOL[dtype]
    yref = y.detach()
    if indexed:
        for k in range(S // Bsz):
            got = out.float().cpu().double()[k * Bsz:(k + 1) * Bsz][:, operm[k].long()]
            torch.testing.assert_close(got, yref[k * Bsz:(k + 1) * Bsz], rtol=rf, atol=af * max(1.0, yref.abs().max().item()))
    else:
        torch.testing.assert_close(out.float().cpu().double(), yref, rtol=rf, atol=af * max(1.0, yref.abs().max().item()))

    def chk(got, ref, name, sum_scale=1.0):
        sc = max(1.0, ref.abs().max().item())
        torch.testing.assert_close(got, ref, rtol=rtol, atol=atol * sc * sum_scale, msg=lambda m: f"{name}: {m}")

    chk(du, u.grad, "du")
    chk(ddelta, dl.grad, "ddelta")
    if indexed and with_z:
        # dz slabs are per direction in token order: sum them
        chk(dz.view(S // Bsz, Bsz, L, Dm).sum(0), z.grad, "dz")
    elif with_z:
        chk(dz, z.grad, "dz")
    # dB / dC are sums over Dm channels, dA / dD / dbias over S*L steps: the absolute floor scales with the root of the count
    wide = max(1.0, (Dm / 128.0) ** 0.5) if dtype != torch.float32 else 1.0
    chk(dB, Bm.grad, "dB", 4.0 * wide)
    chk(dC, Cm.grad, "dC", 4.0 * wide)
    chk(dA, A.grad, "dA", 4.0)
    chk(dD, Dp.grad, "dD", 4.0)
    chk(dbias, bias.grad, "dbias", 4.0)
    # The reduced gradients as WHOLE vectors: the elementwise bound above scales with max|ref| and the channel
    # count and cannot fail for the 16-bit matrix-pipe reduce-scatter of dB / dC (the fp32 instantiation takes the permlane path);
    # a relative L2 error can.  Bounds: the products that enter the dB / dC sums are rounded to the I/O dtype's 8 / 11 bits
    # (independent roundings average down over the channels), the packed bf16 checkpoints carry 2^-9 per state.
    rel_tol = {torch.float32: 2e-4, torch.bfloat16: 2e-2, torch.float16: 4e-3}[dtype]
    for name, got, ref in (("dB", dB, Bm.grad), ("dC", dC, Cm.grad), ("dA", dA, A.grad), ("dD", dD, Dp.grad), ("dbias", dbias, bias.grad)):
        rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
        assert rel <= rel_tol, f"{name}: rel-L2 {rel:.3e} > {rel_tol:.0e} ({dtype}, S={S}, L={L}, D={Dm}, N={N})"


@pytest.mark.parametrize("S,L,Dm", [(2, 196, 256), (3, 49, 128), (2, 16, 64), (1, 13, 200), (2, 1, 64)])
def test_scan_bwd_matches_oracle_autograd(gpu, S, L, Dm):
    _scan_bwd_case(gpu, torch.float32, S, L, Dm, 16, seed=L + Dm)


def test_scan_bwd_no_z(gpu):
    _scan_bwd_case(gpu, torch.float32, 2, 29, 128, 16, seed=9, with_z=False)


def test_scan_bwd_bf16(gpu):
    _scan_bwd_case(gpu, torch.bfloat16, 2, 40, 128, 16, seed=4)


def test_scan_bwd_indexed_three_directions(gpu):
    _scan_bwd_case(gpu, torch.float32, 6, 37, 128, 16, seed=21, indexed=True, Bsz=2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("L", [196, 49])
def test_scan_bwd_bench_instantiation(gpu, dtype, L):
    """The instantiation bench.py times: D = 1024 (4 waves x 4 workgroups per sequence, the bf16 path
    sums dB/dC on the matrix pipe), 3 directions through row-index tables sharing z and the merged dout, checkpoints in the
    dtype's own format -- backward AND forward of that launch against fp64 autograd of the oracle."""
    _scan_bwd_case(gpu, dtype, 6, L, 1024, 16, seed=100 + L, indexed=True, Bsz=2)


# The K2c instantiations the rows below leave out, at the smallest shapes that cross chunks and leave ragged tails: 72 channels (one
# full and one partial wave), L = 20 (8 steps per wave: three chunks, the last sub-chunk partial) and L = 60 (28 steps per wave:
# three chunks).  Gate x row tables x delta mode 0 / 1 x the one-exp form, each at both chunk lengths.
_K2C_GATE_IDX = [dict(), dict(with_z=False), dict(indexed=True, Bsz=1), dict(indexed=True, Bsz=1, with_z=False)]
_K2C_REST = ([(2, 20, 72, dict(with_z=False)), (3, 20, 72, dict(indexed=True, Bsz=1, with_z=False)), (3, 60, 72, dict(indexed=True, Bsz=1, with_z=False)),
              (3, 20, 72, dict(indexed=True, Bsz=1, a_shared=True, dout_per_seq=True))]
             + [(3, L, 72, dict(delta_softplus=False, **kw)) for L in (20, 60) for kw in _K2C_GATE_IDX])
# ... and all of them with fp32 B / C next to 16-bit I/O
_K2C_FP32_BC = [(3, L, 72, dict(bc_fp32=True, delta_softplus=sp, **kw)) for L in (20, 60) for sp in (True, False) for kw in _K2C_GATE_IDX] + \
               [(3, L, 72, dict(bc_fp32=True, indexed=True, Bsz=1, a_shared=True, dout_per_seq=True)) for L in (20, 60)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("S,L,Dm,kw", [
    (6, 196, 1024, dict(indexed=True, Bsz=2)),                    # the model's call at batch 2: 7 waves x 28 steps
    (3, 183, 128, dict(indexed=True, Bsz=1)),                     # ragged: the last chunk is partial, and so is its last sub-chunk
    (2, 196, 200, dict()),                                        # no index tables, ragged channel count
    (2, 100, 64, dict(with_z=False)),                             # chunks past the end of the sequence, no gate
    (6, 49, 256, dict(indexed=True, Bsz=2)),                      # L = 49 (DiffMa-*/4): 7 waves x 8 steps
    (2, 30, 128, dict()),
    (3, 196, 256, dict(indexed=True, Bsz=1, a_shared=True, dout_per_seq=True)),   # the Mamba-2 call pattern
] + _K2C_REST)
def test_scan_bwd_chunk_parallel_variant(gpu, dtype, S, L, Dm, kw):
    """K2c (csrc/scan_bwd_chunked.h): NW waves per (sequence, 64 channels), two passes joined by the linearity of the adjoint
    carry -- every gradient against fp64 autograd of the oracle, same tolerances as the sequential kernel."""
    _scan_bwd_case(gpu, dtype, S, L, Dm, 16, seed=7 * L + Dm, variant="chunked", **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("S,L,Dm,kw", _K2C_FP32_BC)
def test_scan_bwd_chunk_parallel_fp32_bc(gpu, dtype, S, L, Dm, kw):
    """K2c with fp32 B / C and 16-bit I/O: _scan_bwd_case, same checks and tolerances."""
    _scan_bwd_case(gpu, dtype, S, L, Dm, 16, seed=7 * L + Dm, variant="chunked", **kw)


def test_scan_bwd_variants_agree_and_default_choice(gpu):
    """The library's own choice: a small launch takes the chunk-parallel kernel (partial rows per 64 channels), a large one the
    sequential kernel (per 256); both give the same gradients up to fp32 summation order."""
    from diffma_amd import _lib, hip_ops

    lib = _lib.load()
    assert lib.dm_scan_bwd_launch_group_channels(24, 1024, 196, 16, 0) == 64
    assert lib.dm_scan_bwd_launch_group_channels(768, 1024, 196, 16, 0) == 256
    assert lib.dm_scan_bwd_launch_group_channels(24, 1024, 196, 16, _lib.DM_FLAG_SCAN_SEQUENTIAL) == 256
    assert lib.dm_scan_bwd_launch_group_channels(24, 1024, 16, 16, 0) == 256          # too short to cut
    S, L, Dm, N = 4, 196, 256, 16
    host, d = _inputs(S, L, Dm, N, torch.float32, seed=77, dev=gpu)
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, torch.float32, gpu)
    hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["bias"], True, ckpt=ckpt)
    dout = torch.randn(S, L, Dm, generator=torch.Generator().manual_seed(3)).to(gpu)
    ra = hip_ops.scan_bwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["bias"], dout, ckpt, True, variant="sequential")
    rb = hip_ops.scan_bwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["bias"], dout, ckpt, True)      # library's choice: chunked
    for name, x0, x1 in zip(("du", "ddelta", "dz", "dB", "dC", "dA", "dD", "dbias"), ra, rb):
        torch.testing.assert_close(x1, x0, rtol=2e-4, atol=2e-5 * max(1.0, x0.abs().max().item()), msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("variant", ["sequential", "chunked"])
@pytest.mark.parametrize("S,L,kw", [(3, 196, dict(indexed=True, Bsz=1)), (3, 183, dict())], ids=["196-indexed", "183"])
def test_scan_bwd_long_memory(gpu, dtype, variant, S, L, kw):
    """_scan_bwd_case, unchanged checks and tolerances, on _inputs_long_memory: the chunk fold, the checkpoint recompute and the
    dA / d delta reverse sums carry O(1) state over the whole sequence (with _inputs, whatever crosses two chunks is 1e-10)."""
    _scan_bwd_case(gpu, dtype, S, L, 128, 16, seed=11 * L, variant=variant, long_memory=True, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_scan_bwd_long_memory_a_shared_dout_per_seq(gpu, dtype):
    """The Mamba-2 call pattern (one decay per channel in [-16, -0.16], per-direction gradients) where the state remembers."""
    _scan_bwd_case(gpu, dtype, 3, 196, 128, 16, seed=1961, indexed=True, Bsz=1, a_shared=True, dout_per_seq=True, variant="chunked", long_memory=True)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_scan_bwd_16bit_plain(gpu, dtype):
    _scan_bwd_case(gpu, dtype, 2, 40, 128, 16, seed=4)
    _scan_bwd_case(gpu, dtype, 3, 29, 200, 16, seed=5, with_z=False)          # ragged channel count, no gate


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scan_bwd_a_shared_dout_per_seq(gpu, dtype):
    """DM_FLAG_A_SHARED + DM_FLAG_DOUT_PER_SEQ at kernel level: the Mamba-2 call pattern of _SpiralSSDFn (one decay per
    channel, per-direction gradients read through the scatter table)."""
    _scan_bwd_case(gpu, dtype, 6, 49, 256, 16, seed=31, indexed=True, Bsz=2, a_shared=True, dout_per_seq=True)
    _scan_bwd_case(gpu, dtype, 3, 196, 1024, 16, seed=32, indexed=True, Bsz=1, a_shared=True, dout_per_seq=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scan_bwd_dout_per_seq_without_a_shared(gpu, dtype):
    _scan_bwd_case(gpu, dtype, 4, 37, 128, 16, seed=33, indexed=True, Bsz=2, dout_per_seq=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [8, 32])
def test_scan_bwd_other_dstate(gpu, dtype, N):
    """The d_state 8 and 32 instantiations of the backward (scan_bwd_impl.h: 32 runs two lanes per channel)."""
    _scan_bwd_case(gpu, dtype, 2, 21, 128, N, seed=N)
    _scan_bwd_case(gpu, dtype, 4, 40, 200, N, seed=N + 1, indexed=True, Bsz=2)


@pytest.mark.parametrize("Bsz,L,Dm,W", [(2, 196, 256, 4), (2, 30, 128, 4), (1, 5, 200, 3), (1, 1, 64, 4)])
def test_gather_conv_bwd_matches_oracle_autograd(gpu, Bsz, L, Dm, W):
    from diffma_amd import hip_ops
    from oracle.mamba_ref import causal_conv1d_ref

    g = torch.Generator().manual_seed(L + Dm + W)
    xz = torch.randn(Bsz, L, 2 * Dm, generator=g)
    w = torch.randn(Dm, W, generator=g) * 0.5
    b = torch.randn(Dm, generator=g) * 0.1
    ndir = 3
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    dout = torch.randn(ndir * Bsz, L, Dm, generator=g)
    dx, dw, db = hip_ops.gather_conv1d_bwd(xz.to(gpu)[..., :Dm], w.to(gpu), b.to(gpu), dout.to(gpu),
                                          row_index=perms.to(gpu), ndir=ndir)
    torch.cuda.synchronize()
    x = xz[..., :Dm].double().clone().requires_grad_(True)
    wd, bd = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    loss = 0
    for k in range(ndir):
        xs = x[:, perms[k].long(), :]
        y = causal_conv1d_ref(xs.permute(0, 2, 1), wd, bd, activation="silu").permute(0, 2, 1)
        loss = loss + (y * dout.view(ndir, Bsz, L, Dm)[k].double()).sum()
    loss.backward()
    torch.testing.assert_close(dx.cpu().double().view(ndir, Bsz, L, Dm).sum(0), x.grad, rtol=1e-4, atol=1e-5)
    sc = max(1.0, wd.grad.abs().max().item())
    torch.testing.assert_close(dw.cpu().double(), wd.grad, rtol=1e-4, atol=2e-5 * sc)
    torch.testing.assert_close(db.cpu().double(), bd.grad, rtol=1e-4, atol=2e-5 * sc)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,rows", [(1024, 70), (2304, 33), (200, 5)])
def test_rmsnorm_merge_matches_torch(gpu, dtype, C, rows):
    """Mamba-2 epilogue (csrc/rmsnorm.hip): w * sum_k RMSNorm(y_k), forward and backward vs fp64 autograd of the formula the
    reference's gated RMSNorm applies per direction (block/mamba2.py:349; gate already applied by the scan)."""
    from diffma_amd import hip_ops

    K, Bsz, eps = 3, 1, 1e-5
    g = torch.Generator().manual_seed(C + rows)
    y = torch.randn(K, Bsz, rows, C, generator=g).to(dtype)
    w = torch.randn(C, generator=g)
    dout = torch.randn(Bsz, rows, C, generator=g).to(dtype)
    out, rstd = hip_ops.rmsnorm_merge_fwd(y.to(gpu), w.to(gpu), eps)
    dy, dw = hip_ops.rmsnorm_merge_bwd(y.to(gpu), w.to(gpu), eps, rstd, dout.to(gpu))
    torch.cuda.synchronize()
    yr = y.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    ref = (yr * torch.rsqrt(yr.pow(2).mean(-1, keepdim=True) + eps)).sum(0) * wr
    ref.backward(dout.double())
    rtol, atol = TOL[dtype]
    sc = lambda t: atol * max(1.0, t.abs().max().item())
    torch.testing.assert_close(out.float().cpu().double(), ref.detach(), rtol=rtol, atol=sc(ref.detach()))
    torch.testing.assert_close(dy.float().cpu().double(), yr.grad, rtol=rtol, atol=sc(yr.grad))
    torch.testing.assert_close(dw.cpu().double(), wr.grad, rtol=max(rtol, 1e-3), atol=sc(wr.grad))


@pytest.mark.parametrize("R,C", [(1536, 16384), (37, 1024), (5, 4), (96, 200), (5376, 2560), (5376, 10240), (768, 288), (1000, 1024), (272, 512)])
def test_colsum_matches_torch(gpu, R, C):
    """dm_colsum_f32 (reduces the scan backward's per-sequence dA / dD / dbias partial rows) vs an fp64 sum; the tall, narrow
    shapes (the conv backward's dw / db partial rows at the Mamba-2 width, 768 x 7 rows) take the wrapper's row-class split
    (two launches), odd row counts a smaller split or none; exact on integers, and the same bits launch after launch."""
    from diffma_amd import hip_ops

    x = torch.randn(R, C, generator=torch.Generator().manual_seed(R + C))
    xd = x.to(gpu)
    got = hip_ops.colsum(xd)
    ref = x.double().sum(0)
    torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-5, atol=1e-5 * max(1.0, ref.abs().max().item()))
    assert torch.equal(got, hip_ops.colsum(xd))
    xi = torch.randint(-8, 9, (R, C), generator=torch.Generator().manual_seed(R)).float()
    assert torch.equal(hip_ops.colsum(xi.to(gpu)).cpu(), xi.sum(0))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L,H,ndir,with_z", [(2, 196, 2, 3, True), (1, 49, 4, 3, True), (2, 16, 1, 1, True), (1, 33, 2, 2, False), (1, 1, 1, 1, True),
                                                 (1, 224, 1, 1, True)])
def test_ssd_fwd_mfma_matches_oracle(gpu, dtype, Bsz, L, H, ndir, with_z):
    """K6 (csrc/ssd.hip): Mamba-2 single-chunk SSD on the matrix pipe against the sequential fp64 restatement
    (oracle/mamba2_ref.ssd_scan_ref, pinned by G10's Mamba2.step cases) on the ROUNDED inputs, incl. the in-kernel softplus of
    the per-head dt, the z gather / output scatter tables, ragged L, and against the A-shared scan kernel on the same data."""
    from diffma_amd import hip_ops
    from oracle.mamba2_ref import ssd_scan_ref
    from oracle.mamba_ref import softplus_ref

    P, N = 64, 16
    Din, S = H * P, Bsz * ndir
    g = torch.Generator().manual_seed(L * 11 + H + ndir)
    xBC = torch.randn(S, L, Din + 2 * N, generator=g).to(dtype)
    dt_tok = (torch.randn(Bsz, L, H, generator=g) * 0.7 - 1.0).to(dtype)
    ztok = torch.randn(Bsz, L, Din, generator=g).to(dtype) if with_z else None
    A_h = -(torch.rand(H, generator=g) * 6 + 0.3)
    D_h, bias_h = torch.randn(H, generator=g), torch.randn(H, generator=g) * 0.5
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    dev = lambda t: None if t is None else t.to(gpu)
    xb = dev(xBC)
    out = hip_ops.ssd_fwd(xb[..., :Din], xb[..., Din:Din + N], xb[..., Din + N:], dev(dt_tok), dev(ztok), dev(A_h), dev(D_h), dev(bias_h),
                          z_row_index=dev(perms), out_row_index=dev(perms), batch_per_dir=Bsz)
    torch.cuda.synchronize()
    out = out.float().cpu().double()
    rtol, atol = TOL[dtype]
    for s_ in range(S):
        k, b = divmod(s_, Bsz)
        idx = perms[k].long()
        xs = xBC[s_:s_ + 1].float().double()
        dt = softplus_ref(dt_tok[b][idx].float().double() + bias_h.double())[None]                  # [1, L, H] in scan order
        y = ssd_scan_ref(xs[..., :Din], dt, A_h.double(), xs[..., Din:Din + N], xs[..., Din + N:], D_h.double(), P)[0]      # [L, Din]
        if with_z:
            zz = ztok[b][idx].float().double()
            y = y * (zz * torch.sigmoid(zz))
        got = out[s_][idx]                                                                           # row idx[l] holds step l
        torch.testing.assert_close(got, y, rtol=rtol, atol=atol * max(1.0, y.abs().max().item()), msg=lambda m, s_=s_: f"seq {s_}: {m}")
    if with_z:                  # the A-shared scan on the same inputs (delta expanded per channel, as _SpiralSSDFn does when training)
        idx64 = perms.long().to(gpu)
        dtg = torch.stack([dev(dt_tok)[:, idx64[k]] for k in range(ndir)]).reshape(S, L, H, 1).expand(S, L, H, P).reshape(S, L, Din)
        A = dev(A_h).repeat_interleave(P)[:, None].expand(Din, N).contiguous()
        ref2 = hip_ops.scan_fwd(xb[..., :Din], dtg.contiguous(), A, xb[..., Din:Din + N], xb[..., Din + N:], dev(D_h).repeat_interleave(P), dev(ztok),
                                dev(bias_h).repeat_interleave(P), True, z_row_index=dev(perms), out_row_index=dev(perms), batch_per_dir=Bsz,
                                a_shared=True)
        sc = max(1.0, ref2.float().abs().max().item())
        torch.testing.assert_close(out.float(), ref2.float().cpu(), rtol=rtol, atol=atol * sc)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L,H,ndir", [(2, 196, 2, 3), (1, 49, 3, 3), (2, 16, 1, 1), (1, 33, 2, 2), (1, 1, 1, 1), (1, 64, 1, 2), (1, 130, 2, 1)])
def test_ssd_bwd_mfma_matches_oracle_autograd(gpu, dtype, Bsz, L, H, ndir):
    """K6b (csrc/ssd_bwd.hip): every gradient of the Mamba-2 single-chunk SSD core against fp64 autograd through the sequential
    restatement (oracle/mamba2_ref.ssd_scan_ref, pinned by G10) on the ROUNDED inputs: dx (scan order), dz and d(raw dt) (token
    order per direction, through the row tables), dB / dC (per-head partials summed), dA, dD, d(dt_bias); ragged L, 1..3 directions."""
    from diffma_amd import hip_ops
    from oracle.mamba2_ref import ssd_scan_ref
    from oracle.mamba_ref import softplus_ref

    P, N = 64, 16
    Din, S = H * P, Bsz * ndir
    g = torch.Generator().manual_seed(L * 13 + H * 3 + ndir)
    xBC = torch.randn(S, L, Din + 2 * N, generator=g).to(dtype)
    dt_tok = (torch.randn(Bsz, L, H, generator=g) * 0.7 - 1.0).to(dtype)
    ztok = torch.randn(Bsz, L, Din, generator=g).to(dtype)
    dout = torch.randn(S, L, Din, generator=g).to(dtype)
    A_h = -(torch.rand(H, generator=g) * 6 + 0.3)
    D_h, bias_h = torch.randn(H, generator=g), torch.randn(H, generator=g) * 0.5
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    dev = lambda t: t.to(gpu)
    xb = dev(xBC)
    dxBC = torch.full((S, L, Din + 2 * N), float("nan"), dtype=dtype, device=gpu)       # dx lands in a strided view, as in the mixer
    dx, dz, dbc, ddt, dad = hip_ops.ssd_bwd(xb[..., :Din], xb[..., Din:Din + N], xb[..., Din + N:], dev(dt_tok), dev(ztok), dev(dout), dev(A_h),
                                            dev(D_h), dev(bias_h), z_row_index=dev(perms), out_row_index=dev(perms), batch_per_dir=Bsz,
                                            dx_out=dxBC[..., :Din])
    torch.cuda.synchronize()
    assert dx.data_ptr() == dxBC.data_ptr() and torch.isnan(dxBC[..., Din:].float()).all()

    d64 = lambda t: t.float().double()
    A_r, D_r, b_r = (t.double().requires_grad_(True) for t in (A_h, D_h, bias_h))
    leaves = []
    loss = 0.0
    for s_ in range(S):
        k, b = divmod(s_, Bsz)
        idx = perms[k].long()
        xs = d64(xBC[s_, :, :Din]).requires_grad_(True)
        Bs = d64(xBC[s_, :, Din:Din + N]).requires_grad_(True)
        Cs = d64(xBC[s_, :, Din + N:]).requires_grad_(True)
        raw = d64(dt_tok[b]).requires_grad_(True)                                           # token order, one leaf per sequence
        zz = d64(ztok[b]).requires_grad_(True)
        dt = softplus_ref(raw[idx] + b_r)[None]
        y = ssd_scan_ref(xs[None], dt, A_r, Bs[None], Cs[None], D_r, P)[0]
        zg = zz[idx]
        out = y * (zg * torch.sigmoid(zg))
        loss = loss + (out * d64(dout[s_])[idx]).sum()                                       # step l's gradient sits at row idx[l]
        leaves.append((xs, Bs, Cs, raw, zz))
    loss.backward()

    rtol, atol = TOL[dtype]

    def close(got, ref, what, slack=1.0):
        got = got.float().cpu().double()
        torch.testing.assert_close(got, ref, rtol=rtol * slack, atol=atol * slack * max(1.0, ref.abs().max().item()), msg=lambda m: f"{what}: {m}")

    close(dx, torch.stack([lv[0].grad for lv in leaves]), "dx")
    close(dz, torch.stack([lv[4].grad for lv in leaves]), "dz")
    close(ddt, torch.stack([lv[3].grad for lv in leaves]), "d raw dt")
    close(dbc[..., :N], torch.stack([lv[1].grad for lv in leaves]), "dB")
    close(dbc[..., N:], torch.stack([lv[2].grad for lv in leaves]), "dC")
    close(dad[0], A_r.grad, "dA")
    close(dad[1], D_r.grad, "dD")
    close(dad[2], b_r.grad, "d dt_bias")
    close(ddt.sum((0, 1)), b_r.grad, "d dt_bias (sum of d raw dt)")


def test_ssd_matrix_pipe_agrees_with_the_scan_pair_at_full_size(gpu):
    """BASELINE config 4 at full size (DiffMa-XL/2 --use-mamba2, batch 64: 192 gathered sequences x 16 heads x 196 steps): the
    matrix-pipe pair (K6 / K6b) against the A-shared scan pair (K1 / K2) -- two independent HIP implementations of the same
    operator, each pinned to the oracle at small sizes -- on every output; exercises the grid-level indexing (head column
    offsets, per-direction row tables, batch_per_dir sharing of z and dt) that the small cases cannot."""
    from diffma_amd import hip_ops

    B, L, H, P, N, ndir = 64, 196, 16, 64, 16, 3
    S, Din = ndir * B, H * P
    dt_ = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(77)
    xBC = torch.randn(S, L, Din + 2 * N, generator=g).to(dt_).to(gpu)
    dt_tok = (torch.randn(B, L, H, generator=g) * 0.7 - 1.0).to(dt_).to(gpu)
    z = torch.randn(B, L, Din, generator=g).to(dt_).to(gpu)
    dout = torch.randn(S, L, Din, generator=g).to(dt_).to(gpu)
    A_h = -(torch.rand(H, generator=g) * 6 + 0.3).to(gpu)
    D_h, b_h = torch.randn(H, generator=g).to(gpu), (torch.randn(H, generator=g) * 0.5).to(gpu)
    idx = torch.stack([torch.arange(L), torch.randperm(L, generator=g), torch.randperm(L, generator=g)]).int().to(gpu)
    x, Bm, Cm = xBC[..., :Din], xBC[..., Din:Din + N], xBC[..., Din + N:]

    y1 = hip_ops.ssd_fwd(x, Bm, Cm, dt_tok, z, A_h, D_h, b_h, z_row_index=idx, out_row_index=idx, batch_per_dir=B)
    dxBC1 = torch.empty_like(xBC)
    _, dz1, dbc1, ddt1, dad1 = hip_ops.ssd_bwd(x, Bm, Cm, dt_tok, z, dout, A_h, D_h, b_h, z_row_index=idx, out_row_index=idx,
                                               batch_per_dir=B, dx_out=dxBC1[..., :Din])
    idx64 = idx.long()
    inv = torch.argsort(idx64, dim=1)
    delta = torch.stack([dt_tok[:, idx64[k]] for k in range(ndir)]).reshape(S, L, H, 1).expand(S, L, H, P).reshape(S, L, Din).contiguous()
    A = A_h.repeat_interleave(P)[:, None].expand(Din, N).contiguous()
    Dp, bp = D_h.repeat_interleave(P), b_h.repeat_interleave(P)
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Din, dt_, gpu)
    y2 = hip_ops.scan_fwd(x, delta, A, Bm, Cm, Dp, z, bp, True, z_row_index=idx, out_row_index=idx, batch_per_dir=B, ckpt=ckpt, a_shared=True)
    dxBC2 = torch.empty_like(xBC)
    _, ddelta, dz2, _, _, dA2, dD2, dbias2 = hip_ops.scan_bwd(x, delta, A, Bm, Cm, Dp, z, bp, dout, ckpt, True, z_row_index=idx, out_row_index=idx,
                                                             batch_per_dir=B, dout_per_seq=True, du_out=dxBC2[..., :Din], a_shared=True,
                                                             dbc_out=dxBC2[..., Din:])
    torch.cuda.synchronize()

    def agree(a, b, what, tol=2e-2):
        a, b = a.float(), b.float()
        err = (a - b).norm() / b.norm().clamp_min(1e-30)
        assert torch.isfinite(a).all() and err <= tol, (what, float(err))

    agree(y1, y2, "out")
    agree(dxBC1[..., :Din], dxBC2[..., :Din], "dx")
    agree(dz1, dz2, "dz")
    agree(dbc1, dxBC2[..., Din:], "dB | dC")
    # the scan pair returns d(delta) per channel in scan order: sum the head's channels and put the rows in token order
    ddt2 = ddelta.float().view(ndir, B, L, H, P).sum(-1)
    ddt2 = torch.stack([ddt2[k][:, inv[k]] for k in range(ndir)]).reshape(S, L, H)
    agree(ddt1, ddt2, "d raw dt")
    agree(dad1[0], dA2.float().view(H, P * N).sum(-1), "dA")
    agree(dad1[1], dD2.float().view(H, P).sum(-1), "dD")
    agree(dad1[2], dbias2.float().view(H, P).sum(-1), "d dt_bias")


# ------------------------------------------------------------------------------------------------------------------
# Round 3: the SiLU(z) gate and the softplus hoisted out of the per-direction scans (block/mamba.py:41-45,66-68,346-348)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L,Dm,K", [(2, 49, 128, 3), (1, 7, 200, 2), (2, 196, 1024, 3)])
def test_token_merge_gated(gpu, dtype, Bsz, L, Dm, K):
    """out = silu(z) * sum_k slab_k with z read from the strided z half of an xz buffer; `pre` = the ungated sum in the I/O dtype,
    and the gate is applied to the ROUNDED sum (what the backward reads back)."""
    from diffma_amd import hip_ops

    g = torch.Generator().manual_seed(L + Dm)
    slabs = torch.randn(K, Bsz, L, Dm, generator=g).to(dtype)
    xz = torch.randn(Bsz, L, 2 * Dm, generator=g).to(dtype)
    xz_d = xz.to(gpu)
    pre = torch.empty(Bsz, L, Dm, dtype=dtype, device=gpu)
    out = hip_ops.token_merge(slabs.to(gpu), gate=xz_d[..., Dm:], pre_out=pre)
    s = slabs.float()
    acc = s[0]
    for k in range(1, K):
        acc = acc + s[k]
    pre_ref = acc.to(dtype)
    assert torch.equal(pre.cpu(), pre_ref)                                    # same summation order, one rounding
    z = xz[..., Dm:].double()
    ref = pre_ref.double() * z * torch.sigmoid(z)
    rtol, atol = {torch.float32: (2e-6, 1e-6), torch.bfloat16: (1e-2, 1e-3), torch.float16: (2e-3, 1e-4)}[dtype]
    torch.testing.assert_close(out.cpu().double(), ref, rtol=rtol, atol=atol)
    out2 = hip_ops.token_merge(slabs.to(gpu), gate=xz_d[..., Dm:])           # without pre: the fp32 sum is gated
    ref2 = acc.double() * z * torch.sigmoid(z)
    torch.testing.assert_close(out2.cpu().double(), ref2, rtol=rtol, atol=atol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L,Dm", [(2, 49, 128), (1, 7, 200), (2, 196, 1024)])
def test_gate_bwd_matches_autograd(gpu, dtype, Bsz, L, Dm):
    from diffma_amd import hip_ops

    g = torch.Generator().manual_seed(3 * L + Dm)
    dy = torch.randn(Bsz, L, Dm, generator=g).to(dtype)
    pre = torch.randn(Bsz, L, Dm, generator=g).to(dtype)
    xz = torch.randn(Bsz, L, 2 * Dm, generator=g).to(dtype)
    dxz = torch.zeros(Bsz, L, 2 * Dm, dtype=dtype, device=gpu)
    gd, dz = hip_ops.gate_bwd(dy.to(gpu), xz.to(gpu)[..., Dm:], pre.to(gpu), dz_out=dxz[..., Dm:])
    z = xz[..., Dm:].double().clone().requires_grad_(True)
    p = pre.double().clone().requires_grad_(True)
    (p * torch.nn.functional.silu(z) * dy.double()).sum().backward()
    rtol, atol = {torch.float32: (1e-5, 1e-6), torch.bfloat16: (1e-2, 2e-3), torch.float16: (2e-3, 2e-4)}[dtype]
    torch.testing.assert_close(gd.cpu().double(), p.grad, rtol=rtol, atol=atol)
    torch.testing.assert_close(dxz[..., Dm:].cpu().double(), z.grad, rtol=rtol, atol=atol)
    assert dz.data_ptr() == dxz[..., Dm:].data_ptr() and float(dxz[..., :Dm].abs().max()) == 0.0   # only the z half is written


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,Dm,R,P", [(2 * 196 * 3, 1024, 32, 64), (70, 208, 16, 48), (33, 64, 8, 40), (16 * 9 + 5, 1536, 24, 56)])
def test_dtproj_softplus_matches_torch(gpu, dtype, M, Dm, R, P):
    """delta = softplus(x_dbl[:, :R] @ W^T + bias) from the rank-R MFMA kernel (ragged row counts, widths that are not a multiple of
    the 512-column workgroup, ranks below the MFMA K) against fp64; extreme pre-activations cover the three softplus branches."""
    from diffma_amd import hip_ops

    g = torch.Generator().manual_seed(M + Dm + R)
    xdbl = torch.randn(M, P, generator=g).to(dtype)
    w = (torch.randn(Dm, R, generator=g) * R ** -0.5).to(dtype)
    bias = torch.randn(Dm, generator=g)
    bias[:4] = torch.tensor([30.0, -30.0, -12.0, 19.0])
    xd, wd = xdbl.to(gpu), w.to(gpu)
    assert hip_ops.dtproj_softplus_supported(xd, wd)
    delta = hip_ops.dtproj_softplus_fwd(xd, wd, bias.to(gpu))
    ref = torch.nn.functional.softplus(xdbl[:, :R].double() @ w.double().t() + bias.double(), threshold=20.0)
    rtol, atol = {torch.bfloat16: (1e-2, 1e-6), torch.float16: (2e-3, 1e-6)}[dtype]
    torch.testing.assert_close(delta.cpu().double(), ref, rtol=rtol, atol=atol)


def _hoisted_scan_case(gpu, dtype, Bsz, L, Dm, ndir, variant, seed, long_memory=False, bc_fp32=False):
    """The DiffMa mixer's call pattern after the hoists: no z, row-index tables, delta already activated (DM_FLAG_DELTA_ACTIVATED),
    the pre-gated gradient shared by the directions.  Forward and backward against fp64 autograd of the oracle run on the SAME
    activated delta; ddelta / dbias must be the gradients of the RAW pre-activation, i.e. times 1 - exp(-delta)."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import selective_scan_ref

    N, S = 16, ndir * Bsz
    host, d = (_inputs_long_memory if long_memory else _inputs)(S, L, Dm, N, dtype, seed=seed, dev=gpu, with_z=False)
    if bc_fp32:                            # fp32 B / C tensors (values rounded to dtype) next to 16-bit I/O
        d["B"], d["C"] = host["B"].float().to(gpu), host["C"].float().to(gpu)
    g = torch.Generator().manual_seed(seed + 1)
    act = torch.nn.functional.softplus(host["delta"].float() + host["bias"]).to(dtype)      # what dm_dtproj_softplus_fwd would hand over
    perm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)]).int()
    dout = torch.randn(Bsz, L, Dm, generator=g).to(dtype)
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dtype, gpu).zero_()
    kw = dict(z_row_index=perm.to(gpu), out_row_index=perm.to(gpu), batch_per_dir=Bsz, variant=variant, delta_activated=True)
    fwd_variant = variant if (variant != "chunked" or 16 * 14 // 4 < L <= 196) else "sequential"
    out = hip_ops.scan_fwd(d["u"], act.to(gpu), d["A"], d["B"], d["C"], d["D"], None, d["bias"], True, ckpt=ckpt,
                           **{**kw, "variant": fwd_variant})
    res = hip_ops.scan_bwd(d["u"], act.to(gpu), d["A"], d["B"], d["C"], d["D"], None, d["bias"], dout.to(gpu), ckpt, True, **kw)
    torch.cuda.synchronize()
    du, ddelta, dz, dB, dC, dA, dD, dbias = [None if t is None else t.float().cpu().double() for t in res]
    assert dz is None

    odev = _oracle_device(gpu, S * L * Dm)
    leaf = lambda t: t.float().double().to(odev).clone().requires_grad_(True)
    u, dl, A, Bm, Cm, Dp = leaf(host["u"]), leaf(act), leaf(host["A"]), leaf(host["B"]), leaf(host["C"]), leaf(host["D"])
    cm = lambda t: t.permute(0, 2, 1)
    y = cm(selective_scan_ref(cm(u), cm(dl), A, cm(Bm), cm(Cm), Dp, z=None, delta_bias=None, delta_softplus=False))
    merged = torch.zeros(Bsz, L, Dm, dtype=torch.float64, device=odev)
    for k in range(ndir):
        merged = merged.index_add(1, perm[k].long().to(odev), y[k * Bsz:(k + 1) * Bsz])
    (merged * dout.float().double().to(odev)).sum().backward()
    dl_val = dl.detach().cpu()
    u, dl, A, Bm, Cm, Dp = _grads_to_cpu(u, dl, A, Bm, Cm, Dp)
    rf, af = TOL[dtype]
    yref = y.detach().cpu()
    for k in range(ndir):
        got = out.float().cpu().double()[k * Bsz:(k + 1) * Bsz][:, perm[k].long()]
        torch.testing.assert_close(got, yref[k * Bsz:(k + 1) * Bsz], rtol=rf, atol=af * max(1.0, yref.abs().max().item()))
    rtol, atol = {torch.float32: (2e-4, 2e-5), torch.bfloat16: (4e-2, 6e-2), torch.float16: (5e-3, 8e-3)}[dtype]

    def chk(got, ref, name, sum_scale=1.0):
        sc = max(1.0, ref.abs().max().item())
        torch.testing.assert_close(got, ref, rtol=rtol, atol=atol * sc * sum_scale, msg=lambda m: f"{name}: {m}")

    draw = dl.grad * (1.0 - torch.exp(-dl_val))                                            # chain through softplus: sigmoid(raw)
    wide = max(1.0, (Dm / 128.0) ** 0.5) if dtype != torch.float32 else 1.0
    chk(du, u.grad, "du")
    chk(ddelta, draw, "ddelta (raw)")
    chk(dB, Bm.grad, "dB", 4.0 * wide)
    chk(dC, Cm.grad, "dC", 4.0 * wide)
    chk(dA, A.grad, "dA", 4.0)
    chk(dD, Dp.grad, "dD", 4.0)
    chk(dbias, draw.sum((0, 1)), "dbias", 4.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L,Dm,ndir,variant", [(2, 196, 1024, 3, "sequential"), (2, 49, 128, 3, "sequential"), (1, 13, 200, 2, "sequential"),
                                                   (2, 196, 128, 3, "chunked"), (1, 100, 200, 3, "chunked"), (2, 49, 128, 3, "chunked")])
def test_scan_hoisted_call_pattern_matches_oracle_autograd(gpu, dtype, Bsz, L, Dm, ndir, variant):
    _hoisted_scan_case(gpu, dtype, Bsz, L, Dm, ndir, variant, seed=7 * L + Dm)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("L", [20, 60])
def test_scan_hoisted_call_pattern_chunked_fp32_bc(gpu, dtype, L):
    """K2c's activated-delta form with fp32 B / C and 16-bit I/O, at both chunk lengths (8 and 28 steps per wave)."""
    _hoisted_scan_case(gpu, dtype, 1, L, 72, 3, "chunked", seed=7 * L + 72, bc_fp32=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("variant", ["sequential", "chunked"])
def test_scan_hoisted_call_pattern_long_memory(gpu, dtype, variant):
    """_hoisted_scan_case at L = 196 on _inputs_long_memory: the same checks and tolerances with the state carried across chunks."""
    _hoisted_scan_case(gpu, dtype, 1, 196, 128, 3, variant, seed=1960, long_memory=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_spiral_ssm_hoisted_equals_in_scan_gate(gpu, dtype, monkeypatch):
    """The fused 3-direction mixer core with the gate / softplus hoisted (default) against the same operator with both evaluated
    inside every scan (DIFFMA_HOIST_GATE=0, the upstream arrangement): outputs and all gradients agree to rounding."""
    from diffma_amd import selective_scan_interface as ssi
    from diffma_amd import tools

    Bsz, L, Din, N, R = 3, 49, 256, 16, 16
    g = torch.Generator().manual_seed(5)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(gpu)
    xz = mk(Bsz, L, 2 * Din).to(dtype)
    conv_w, conv_b = mk(Din, 1, 4, sc=0.5), mk(Din, sc=0.1)
    Wx, Wdt, dt_b = mk(R + 2 * N, Din, sc=Din ** -0.5), mk(Din, R, sc=R ** -0.5), mk(Din, sc=0.5)
    A, Dsk = -(torch.rand(Din, N, generator=g) * 4 + 0.2).to(gpu), mk(Din)
    sp = tools.spiral(7)
    idx = torch.tensor([list(range(L)), sp[0][2], sp[0][3]], dtype=torch.int32, device=gpu)
    dy = mk(Bsz, L, Din).to(dtype)

    def run(hoist):
        monkeypatch.setattr(ssi, "HOIST_GATE", hoist)
        leaves = [t.clone().requires_grad_(True) for t in (xz, conv_w, conv_b, Wx, Wdt, dt_b, A, Dsk)]
        y = ssi.spiral_ssm(*leaves[:6], leaves[6], leaves[7], idx)
        y.backward(dy)
        return [y.detach().float()] + [t.grad.float() for t in leaves]

    a, b = run(True), run(False)
    tol = dict(rtol=2e-4, atol=2e-4) if dtype == torch.float32 else dict(rtol=4e-2, atol=4e-2)
    for name, p, q in zip(["y", "dxz", "dconv_w", "dconv_b", "dWx", "dWdt", "ddt_bias", "dA", "dD"], a, b):
        sc = max(1.0, float(q.abs().max()))
        torch.testing.assert_close(p, q, rtol=tol["rtol"], atol=tol["atol"] * sc, msg=lambda m, name=name: f"{name}: {m}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("slab", ["0", "1"])
@pytest.mark.parametrize("Bsz,L,Dm,ndir", [(2, 196, 1024, 3), (3, 49, 128, 3), (2, 5, 1024, 2), (1, 37, 128, 4), (8, 256, 256, 3),
                                           (16, 100, 128, 1), (40, 49, 1024, 3)])
def test_fused_conv_xproj_bwd_merged_directions(gpu, monkeypatch, dtype, slab, Bsz, L, Dm, ndir):
    """K4x with DM_FLAG_DX_MERGED, both forms -- the whole-sample form (slab 0: one workgroup per sample walks the directions, dx
    accumulates in ONE token-order buffer in HBM) and the slab form (slab 1, sequences up to 256 rows: a workgroup per (sample,
    128 channels), the running sum in LDS, the gathered sequence cut into 8 segments) -- against fp64 autograd (the gradient of x
    summed over the directions), against the per-direction slabs + dm_token_merge, and dw / db from one partial row per sample.  dx
    is a strided view (the x half of d(xz)): the neighbouring z half must stay untouched.  Sequence lengths: the model's 196, one
    with idle waves (5 rows for 8 segments), odd ones, the largest the slab form takes, batches of 8 / 16 (the XCD-aware workgroup
    order) and of 40 at 8 slabs (the slab form is persistent: 256 workgroups, some of which walk through two samples)."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import causal_conv1d_ref

    monkeypatch.setenv("DM_K4X_SLAB", slab)

    P, W = 64, 4
    g = torch.Generator().manual_seed(L * 7 + Dm + ndir)
    xz = torch.randn(Bsz, L, 2 * Dm, generator=g).to(dtype)
    w = torch.randn(Dm, W, generator=g) * 0.5
    b = torch.randn(Dm, generator=g) * 0.1
    wx = (torch.randn(P, Dm, generator=g) * 0.1).to(dtype)
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    du = torch.randn(ndir * Bsz, L, Dm, generator=g).to(dtype)
    dxdbl = torch.randn(ndir * Bsz * L, P, generator=g).to(dtype)
    dxz = torch.full((Bsz, L, 2 * Dm), 7.0, dtype=dtype, device=gpu)
    args = (xz.to(gpu)[..., :Dm], w.to(gpu), b.to(gpu), du.to(gpu), dxdbl.to(gpu), wx.to(gpu).t().contiguous())
    dx, dw, db = hip_ops.gather_conv1d_xproj_bwd(*args, row_index=perms.to(gpu), ndir=ndir, merged_out=dxz[..., :Dm])
    slabs, dw2, db2 = hip_ops.gather_conv1d_xproj_bwd(*args, row_index=perms.to(gpu), ndir=ndir)
    torch.cuda.synchronize()
    assert dx.data_ptr() == dxz.data_ptr() and float((dxz[..., Dm:] - 7.0).abs().max()) == 0.0
    x = xz[..., :Dm].float().double().clone().requires_grad_(True)
    wd, bd = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    loss = 0
    for k in range(ndir):
        y = causal_conv1d_ref(x[:, perms[k].long(), :].permute(0, 2, 1), wd, bd, activation="silu").permute(0, 2, 1)
        loss = loss + (y * du.view(ndir, Bsz, L, Dm)[k].float().double()).sum() \
            + ((y.reshape(-1, Dm) @ wx.float().double().t()) * dxdbl.view(ndir, Bsz * L, P)[k].float().double()).sum()
    loss.backward()
    rtol, atol = {torch.bfloat16: (3e-2, 5e-2), torch.float16: (4e-3, 8e-3)}[dtype]
    sc = max(1.0, x.grad.abs().max().item())
    torch.testing.assert_close(dxz[..., :Dm].float().cpu().double(), x.grad, rtol=rtol, atol=atol * sc)
    merged = hip_ops.token_merge(slabs.view(ndir, Bsz, L, Dm)).float().cpu()
    torch.testing.assert_close(dxz[..., :Dm].float().cpu(), merged, rtol=rtol, atol=atol * sc)
    sc = max(1.0, wd.grad.abs().max().item())
    torch.testing.assert_close(dw.cpu().double(), wd.grad, rtol=rtol, atol=atol * sc * 0.2)
    torch.testing.assert_close(db.cpu().double(), bd.grad, rtol=rtol, atol=atol * sc * 0.2)
    torch.testing.assert_close(dw.cpu(), dw2.cpu(), rtol=1e-4, atol=1e-4 * sc)
    # the reduced gradients by relative L2 as well: sums over >= 100 rows of 16-bit products in fp32 -- the element-wise
    # bound above (1 % of the largest entry) is loose enough to hide one missing row in a sum of a thousand
    l2 = {torch.bfloat16: 5e-3, torch.float16: 1e-3}[dtype]
    assert rel_l2(dw.cpu().double(), wd.grad) <= l2, rel_l2(dw.cpu().double(), wd.grad)
    assert rel_l2(db.cpu().double(), bd.grad) <= l2, rel_l2(db.cpu().double(), bd.grad)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Bsz,L", [(2, 196), (64, 196), (2, 100), (24, 232)])
def test_fused_conv_xproj_bwd_slab_counts_every_row_on_every_launch(gpu, monkeypatch, dtype, Bsz, L):
    """Soak test of the K4x slab form (promoted from tools/dbg_k4x2.py).  Round 4 met an INTERMITTENT miscount:
    with one layout of the per-row table single rows went missing from dw / db in channels 96-127 of a slab, a different row every
    launch, dx untouched.  An element-wise tolerance cannot see one row in 1 176; an exact count can: with
    du == 1, dx_dbl == 0, conv weight 0 and bias 40 (silu'(40) == 1 in fp32) every gathered row adds exactly 1 to db, so
    db[d] == ndir * B * L as an INTEGER for every channel, and dw[d][j] is a fixed fp32 sum of inputs that must come out
    bit-identical launch after launch (the kernel's reduction order is static).  300 launches per case; 14-row tiles (L 196) and
    16-row tiles (L 100, 232), one workgroup stream per slab (B 2) and persistent workgroups walking several samples (B 24, 64)."""
    from diffma_amd import hip_ops

    monkeypatch.setenv("DM_K4X_SLAB", "1")
    Dm, P, ND, W = 1024, 64, 3, 4
    g = torch.Generator().manual_seed(3)
    # inputs exactly representable in 16 bits with exactly representable fp32 partial sums are not needed: bitwise REPEATABILITY is
    # what is asserted for dw, exactness only for db
    xz = torch.zeros(Bsz, L, 2 * Dm, dtype=dtype, device=gpu)
    xz[..., :Dm] = ((torch.arange(L).view(1, L, 1) % 128 + 128 * (torch.arange(Bsz).view(Bsz, 1, 1) % 2)).float() / 256).to(dtype).to(gpu)
    x = xz[..., :Dm]
    w = torch.zeros(Dm, W, device=gpu)
    b = torch.full((Dm,), 40.0, device=gpu)
    wxt = torch.zeros(Dm, P, dtype=dtype, device=gpu)
    idx = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ND - 1)]).int().to(gpu)
    dxd = torch.zeros(ND * Bsz * L, P, dtype=dtype, device=gpu)
    du = torch.ones(ND * Bsz, L, Dm, dtype=dtype, device=gpu)
    dxz = torch.zeros(Bsz, L, 2 * Dm, dtype=dtype, device=gpu)
    want_db = float(ND * Bsz * L)
    ref_dw = ref_dx = None
    bad = []
    for it in range(300):
        dxz.zero_()
        dx, dw, db = hip_ops.gather_conv1d_xproj_bwd(x, w, b, du, dxd, wxt, row_index=idx, ndir=ND, merged_out=dxz[..., :Dm])
        if it == 0:
            ref_dw, ref_dx = dw.clone(), dx.clone()
            # every token is visited once per direction and every row's d(conv input) is the tap sum of ones: taps are 0 -> dx == 0
            assert float(dx.float().abs().max()) == 0.0
            # dw[d][j] = sum over rows of the input W-1-j rows earlier in the gathered order: positive, same for every channel
            assert float(dw.min()) > 0 and float((dw - dw[0:1]).abs().max()) == 0.0
        n_db = int((db != want_db).sum())
        n_dw = int((dw != ref_dw).sum())
        n_dx = int((dx != ref_dx).sum())
        if n_db or n_dw or n_dx:
            bad.append((it, n_db, n_dw, n_dx, (db != want_db).nonzero()[:4].flatten().tolist(), db[db != want_db][:4].tolist()))
    assert not bad, f"{len(bad)} of 300 launches miscounted: {bad[:5]}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("slab", ["0", "1"])
def test_fused_conv_xproj_bwd_merged_weights_in_io_dtype(gpu, monkeypatch, dtype, slab):
    """Conv weights handed over in the I/O dtype (the 16-bit shadows of step_prep) instead of fp32: the kernels widen them on load, so
    with weights that are exactly representable in 16 bits both instantiations must give the same dx bit for bit and the same dw / db."""
    from diffma_amd import hip_ops

    monkeypatch.setenv("DM_K4X_SLAB", slab)
    Bsz, L, Dm, ndir, P, W = 3, 196, 256, 3, 64, 4
    g = torch.Generator().manual_seed(5)
    x = torch.randn(Bsz, L, Dm, generator=g).to(dtype).to(gpu)
    w16 = (torch.randn(Dm, W, generator=g) * 0.5).to(dtype)
    b16 = (torch.randn(Dm, generator=g) * 0.1).to(dtype)
    wxt = (torch.randn(Dm, P, generator=g) * 0.1).to(dtype).to(gpu)
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int().to(gpu)
    du = torch.randn(ndir * Bsz, L, Dm, generator=g).to(dtype).to(gpu)
    dxdbl = torch.randn(ndir * Bsz * L, P, generator=g).to(dtype).to(gpu)
    outs = []
    for wt, bt in ((w16.float(), b16.float()), (w16, b16)):
        dx = torch.zeros(Bsz, L, Dm, dtype=dtype, device=gpu)
        _, dw, db = hip_ops.gather_conv1d_xproj_bwd(x, wt.to(gpu), bt.to(gpu), du, dxdbl, wxt, row_index=perms, ndir=ndir, merged_out=dx)
        outs.append((dx, dw, db))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(outs[0][2], outs[1][2], rtol=1e-6, atol=1e-6)


def test_conv_xproj_bwd_slab_partial_rows_through_the_c_abi(gpu):
    """The slab form of K4x called as a C-ABI client would: dm_gather_conv1d_xproj_bwd_slab() says how many dw | db partial rows carry
    sums (one per persistent workgroup stream); WITHOUT DM_FLAG_PARTIAL_COMPACT the rows of the other samples are zero-filled (a sum
    over all `batch` rows is right), WITH it only the first rows are written.  40 samples x 8 slabs: some workgroups take two samples.
    dx must be the same buffer bit for bit in both calls and equal to the whole-sample form's within one rounding of the running sum."""
    import ctypes
    from diffma_amd import hip_ops, _lib
    from diffma_amd._lib import dm_conv_xproj_bwd_args, DM_FLAG_SILU, DM_FLAG_DX_MERGED, DM_FLAG_PARTIAL_COMPACT

    B, L, Dm, P, ND, W = 40, 49, 1024, 64, 3, 4
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, L, Dm, generator=g).to(dt).to(gpu)
    w, b = (torch.randn(Dm, W, generator=g) * 0.5).to(gpu), (torch.randn(Dm, generator=g) * 0.1).to(gpu)
    wxt = (torch.randn(Dm, P, generator=g) * 0.1).to(dt).to(gpu)
    idx = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ND - 1)]).int().to(gpu)
    du = torch.randn(ND * B, L, Dm, generator=g).to(dt).to(gpu)
    dxd = torch.randn(ND * B * L, P, generator=g).to(dt).to(gpu)

    def run(flags, slab_env, monkey_rows=None):
        part = torch.full((B, Dm * (W + 1)), 777.0, device=gpu)
        dx = torch.zeros(B, L, Dm, dtype=dt, device=gpu)
        a = dm_conv_xproj_bwd_args()
        a.part_ss = Dm * (W + 1)
        a.batch, a.dim, a.seqlen, a.width, a.ndir = B, Dm, L, W, ND
        a.io_dtype, a.w_dtype = hip_ops.dtype_code(x), hip_ops.dtype_code(w)
        a.flags = DM_FLAG_SILU | DM_FLAG_DX_MERGED | flags
        a.nproj = P
        a.x, a.weight, a.bias, a.row_index = x.data_ptr(), w.data_ptr(), b.data_ptr(), idx.data_ptr()
        a.du, a.dxdbl, a.wxt = du.data_ptr(), dxd.data_ptr(), wxt.data_ptr()
        a.dx, a.dw_partial, a.db_partial = dx.data_ptr(), part.data_ptr(), part[:, Dm * W:].data_ptr()
        a.x_sb, a.x_sl, a.x_sd = x.stride()
        a.du_ss, a.du_sl, a.du_sd = du.stride()
        a.dx_ss, a.dx_sl, a.dx_sd = dx.stride()
        a.xd_sr = dxd.stride(0)
        os.environ["DM_K4X_SLAB"] = slab_env
        try:
            rows = int(_lib.load().dm_gather_conv1d_xproj_bwd_slab(ctypes.byref(a), None))
            _lib.call("dm_gather_conv1d_xproj_bwd", a, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            os.environ.pop("DM_K4X_SLAB", None)
        return rows, dx, part

    r0, dx0, p0 = run(0, "0")
    with pytest.raises(_lib.DiffmaHipError, match="PARTIAL_COMPACT"):          # the whole-sample form writes `batch` rows: the flag is refused
        run(DM_FLAG_PARTIAL_COMPACT, "0")
    r1, dx1, p1 = run(0, "1")
    r2, dx2, p2 = run(DM_FLAG_PARTIAL_COMPACT, "1")
    assert r0 == 0 and r1 == r2 == 32                                   # 256 CUs / 8 slabs = 32 streams (<= the 40 samples)
    assert torch.equal(dx1, dx2)
    assert float((p1[r1:] != 0).sum()) == 0 and float((p2[r2:] != 777.0).sum()) == 0 and torch.equal(p1[:r1], p2[:r2])
    torch.testing.assert_close(dx1.float(), dx0.float(), rtol=1.6e-2, atol=1e-2 * float(dx0.float().abs().max()))
    torch.testing.assert_close(p1.sum(0), p0.sum(0), rtol=1e-3, atol=1e-3 * float(p0.sum(0).abs().max()))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,nw,C", [(2 * 196, 4, 32), (37, 1, 32), (5, 16, 64)])
def test_sum_partials_matches_torch(gpu, out_dtype, M, nw, C):
    """dB/dC partial rows summed and placed into a column block of a wider buffer (the d x_dbl columns) in one pass."""
    from diffma_amd import hip_ops

    g = torch.Generator().manual_seed(M + nw)
    parts = torch.randn(M, nw, C, generator=g).to(gpu)
    wide = torch.full((M, 32 + C), 3.0, dtype=out_dtype, device=gpu)
    hip_ops.sum_partials(parts, wide[:, 32:])
    ref = parts.sum(1).to(out_dtype)
    tol = dict(rtol=1e-6, atol=1e-6) if out_dtype == torch.float32 else dict(rtol=8e-3, atol=1e-2)
    torch.testing.assert_close(wide[:, 32:], ref, **tol)
    assert float((wide[:, :32] - 3.0).abs().max()) == 0.0
    out3 = torch.empty(M // 1, C, dtype=out_dtype, device=gpu)
    torch.testing.assert_close(hip_ops.sum_partials(parts, out3), ref, **tol)


# ---- tail of the block's fusion MLP (csrc/gate_head.hip) vs plain PyTorch in fp64 ---------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,C,with_b1,strided", [(3 * 196, 512, True, False), (37, 64, True, True), (5000, 384, False, False),
                                                    (130, 1024, True, False), (64, 2048, True, False), (1, 8, True, False)])
def test_gate_head_matches_torch(gpu, dtype, rows, C, with_b1, strided):
    """a = sigmoid(silu(h + b1) @ w2 + b2) and its backward (dh, db1, dw2, db2): one pass each instead of ATen's bias / SiLU /
    Linear(C, 1) / Sigmoid chain (reference block/mamba_block.py:90-91)."""
    from diffma_amd import hip_ops

    if dtype == torch.float32 and C > 1024:
        pytest.skip("fp32 rows hold at most 1024 values")
    g = torch.Generator().manual_seed(rows + C)
    wide = torch.randn(rows, C + (16 if strided else 0), generator=g).to(dtype)
    h = wide[:, :C]
    b1 = (torch.randn(C, generator=g) * 0.3) if with_b1 else None
    w2 = torch.randn(C, generator=g) / C ** 0.5
    b2 = torch.randn(1, generator=g) * 0.2
    da = torch.randn(rows, 1, generator=g).to(dtype)
    dev = lambda t: None if t is None else t.to(gpu)
    hd = dev(wide)[:, :C]
    assert hip_ops.gate_head_supported(hd)
    a = hip_ops.gate_head_fwd(hd, dev(b1), dev(w2), dev(b2))
    dh, db1, dw2, db2 = hip_ops.gate_head_bwd(dev(da), a, hd, dev(b1), dev(w2))
    torch.cuda.synchronize()

    h64 = h.double().requires_grad_(True)
    b164 = None if b1 is None else b1.double().requires_grad_(True)
    w264, b264 = w2.double().requires_grad_(True), b2.double().requires_grad_(True)
    x = h64 if b164 is None else h64 + b164
    ref = torch.sigmoid(torch.nn.functional.silu(x) @ w264[:, None] + b264)
    ref.backward(da.double())
    rtol, atol = TOL[dtype]
    assert a.shape == (rows, 1) and a.dtype == dtype
    torch.testing.assert_close(a.cpu().double(), ref.detach(), rtol=rtol, atol=atol)
    # the kernel differentiates at ITS (rounded) output a; in 16-bit that rounding is the error floor of the gradients
    gscale = float(h64.grad.abs().max()) + 1e-30
    torch.testing.assert_close(dh.cpu().double(), h64.grad, rtol=rtol, atol=atol * gscale)
    red = lambda got, want: torch.testing.assert_close(got.cpu().double().reshape(want.shape), want, rtol=max(rtol, 2e-3),
                                                       atol=atol * (float(want.abs().max()) + 1e-30))
    if b1 is not None:
        red(db1, b164.grad)
    red(dw2, w264.grad)
    red(db2, b264.grad)


# ---- backward of the dt_proj product: both consumers of d(delta) in one pass (csrc/dtproj.hip, K8b) -------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,Dm,R,N", [(3 * 8 * 196, 1024, 32, 16), (64, 512, 16, 16), (32 * 37, 768, 32, 16), (32, 1024, 16, 8), (9408, 1024, 32, 16),
                                      (3 * 196, 1024, 32, 16), (5, 512, 16, 16), (33, 768, 16, 16), (3 * 3 * 196, 1024, 32, 16)])
def test_dtproj_bwd_matches_torch(gpu, dtype, M, Dm, R, N):
    """dx_dbl[:, :R] = ddelta @ W and dW = ddelta^T @ x_dbl[:, :R] from ONE read of ddelta; the other columns of d(x_dbl) (dB | dC,
    written by the scan backward) must stay untouched."""
    from diffma_amd import hip_ops

    g = torch.Generator().manual_seed(M + Dm + R)
    ddelta = (torch.randn(M, Dm, generator=g) * 0.5).to(dtype)
    xdbl = torch.randn(M, R + 2 * N, generator=g).to(dtype)
    w = (torch.randn(Dm, R, generator=g) / Dm ** 0.5).to(dtype)
    dxdbl = torch.full((M, R + 2 * N), 7.0).to(dtype)
    dd, xd, wd, dxd = ddelta.to(gpu), xdbl.to(gpu), w.to(gpu), dxdbl.to(gpu)
    assert hip_ops.dtproj_bwd_supported(dd, xd, wd, dxd)
    dW = hip_ops.dtproj_bwd(dd, xd, wd, dxd)
    torch.cuda.synchronize()
    ref_dx = ddelta.double() @ w.double()
    ref_dW = ddelta.double().t() @ xdbl[:, :R].double()
    rtol, atol = TOL[dtype]
    torch.testing.assert_close(dxd[:, :R].cpu().double(), ref_dx, rtol=rtol, atol=atol * float(ref_dx.abs().max()))
    assert bool((dxd[:, R:] == 7.0).all())
    assert dW.shape == (Dm, R) and dW.dtype == torch.float32
    torch.testing.assert_close(dW.cpu().double(), ref_dW, rtol=1e-4, atol=1e-5 * float(ref_dW.abs().max()) * max(1.0, M / 1000))


def test_dtproj_bwd_unsupported_shapes_fall_back(gpu):
    from diffma_amd import hip_ops

    mk = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=gpu)
    assert not hip_ops.dtproj_bwd_supported(mk(64, 1536), mk(64, 64), mk(1536, 32), mk(64, 64))              # width not instantiated
    assert not hip_ops.dtproj_bwd_supported(mk(64, 1024, dt=torch.float32), mk(64, 64, dt=torch.float32), mk(1024, 32, dt=torch.float32),
                                            mk(64, 64, dt=torch.float32))
    with pytest.raises(Exception):
        hip_ops.dtproj_bwd(mk(64, 1536), mk(64, 64), mk(1536, 32), mk(64, 64))


# ---- several congruent launches in one (dm_*_n entry points, ABI 25): the two mixers of a block ------------------------------
def test_paired_launches_are_bit_identical_to_separate_ones(gpu):
    """hip_ops.both() queues the launches of two independent, congruent calls and issues each pair as ONE `_n` launch (blockIdx.z
    picks the argument struct).  Every kernel of the small-launch mixer path -- gather + conv forward / backward, dt_proj + softplus
    and its backward, the chunk-parallel scans, gated merge, gate backward, partial-row sums -- must produce exactly the bits of
    two separate launches, and the pair must really share launches (counted at the library call)."""
    from diffma_amd import _lib, hip_ops

    dt = torch.bfloat16
    Bsz, ndir, L, Din, R, N = 2, 3, 196, 512, 16, 16
    S, M = ndir * Bsz, ndir * Bsz * L
    g = torch.Generator(device=gpu).manual_seed(77)
    mk = lambda *s, sc=1.0: torch.randn(*s, device=gpu, generator=g) * sc

    def mixer_inputs():
        idx = torch.stack([torch.arange(L, device=gpu)] + [torch.randperm(L, device=gpu, generator=g) for _ in range(ndir - 1)]).to(torch.int32)
        return dict(xz=mk(Bsz, L, 2 * Din).to(dt), cw=mk(Din, 4, sc=0.4), cb=mk(Din, sc=0.1), Wx=mk(R + 2 * N, Din, sc=Din ** -0.5).to(dt),
                    Wdt=mk(Din, R, sc=0.3).to(dt), bias=mk(Din, sc=0.5), A=-(torch.rand(Din, N, device=gpu, generator=g) * 4 + 0.2), D=mk(Din),
                    idx=idx, dy=mk(Bsz, L, Din).to(dt))

    mix = [mixer_inputs(), mixer_inputs()]

    def run(paired):
        counts = {}
        real_call, real_call_n = _lib.call, _lib.call_n

        def call(name, a, st):
            counts[name] = counts.get(name, 0) + 1
            return real_call(name, a, st)

        def call_n(name, arr, st):
            counts[name] = counts.get(name, 0) + 1
            return real_call_n(name, arr, st)

        _lib.call, _lib.call_n = call, call_n
        try:
            out = [dict(), dict()]

            def stage(fn):
                hip_ops.both(lambda k: fn(mix[k], out[k]), enabled=paired)

            def conv(m, o):
                o["xc"] = hip_ops.gather_conv1d_fwd(m["xz"][..., :Din], m["cw"], m["cb"], row_index=m["idx"], ndir=ndir, silu=True)
            stage(conv)
            for k in (0, 1):
                out[k]["x_dbl"] = (out[k]["xc"].view(M, Din) @ mix[k]["Wx"].t()).contiguous()

            def dtp(m, o):
                o["delta"] = hip_ops.dtproj_softplus_fwd(o["x_dbl"], m["Wdt"], m["bias"]).view(S, L, Din)
            stage(dtp)

            def scan(m, o):
                xd3 = o["x_dbl"].view(S, L, R + 2 * N)
                o["ckpt"] = hip_ops.alloc_scan_ckpt(S, L, N, Din, dt, gpu)
                o["ydir"] = hip_ops.scan_fwd(o["xc"], o["delta"], m["A"], xd3[..., R:R + N], xd3[..., R + N:], m["D"], None, m["bias"], True,
                                             z_row_index=m["idx"], out_row_index=m["idx"], batch_per_dir=Bsz, ckpt=o["ckpt"], delta_activated=True)
            stage(scan)

            def merge(m, o):
                o["pre"] = torch.empty((Bsz, L, Din), dtype=dt, device=gpu)
                o["y"] = hip_ops.token_merge(o["ydir"].view(ndir, Bsz, L, Din), gate=m["xz"][..., Din:], pre_out=o["pre"])
            stage(merge)

            def gate(m, o):
                o["dxz"] = torch.zeros((Bsz, L, 2 * Din), dtype=dt, device=gpu)
                o["g"], _ = hip_ops.gate_bwd(m["dy"], m["xz"][..., Din:], o["pre"], dz_out=o["dxz"][..., Din:])
            stage(gate)

            def bwd(m, o):
                xd3 = o["x_dbl"].view(S, L, R + 2 * N)
                o["dx_dbl"] = torch.zeros((M, R + 2 * N), dtype=dt, device=gpu)
                o["sb"] = hip_ops.scan_bwd(o["xc"], o["delta"], m["A"], xd3[..., R:R + N], xd3[..., R + N:], m["D"], None, m["bias"], o["g"], o["ckpt"],
                                           True, z_row_index=m["idx"], out_row_index=m["idx"], batch_per_dir=Bsz,
                                           dbc_out=o["dx_dbl"].view(S, L, R + 2 * N)[..., R:], delta_activated=True)
            stage(bwd)

            def dtb(m, o):
                o["dWdt"] = hip_ops.dtproj_bwd(o["sb"][1].view(M, Din), o["x_dbl"], m["Wdt"], o["dx_dbl"])
            assert hip_ops.dtproj_bwd_supported(out[0]["sb"][1].view(M, Din), out[0]["x_dbl"], mix[0]["Wdt"], out[0]["dx_dbl"])
            stage(dtb)

            def cbwd(m, o):
                o["cb"] = hip_ops.gather_conv1d_bwd(m["xz"][..., :Din], m["cw"], m["cb"], o["sb"][0], row_index=m["idx"], ndir=ndir, silu=True)
            stage(cbwd)

            def dxm(m, o):
                hip_ops.token_merge(o["cb"][0].view(ndir, Bsz, L, Din), out=o["dxz"][..., :Din])
            stage(dxm)
            torch.cuda.synchronize()
            return out, counts
        finally:
            _lib.call, _lib.call_n = real_call, real_call_n

    ref, c_ref = run(False)
    got, c_got = run(True)

    def flat(o):
        res = dict(xc=o["xc"], delta=o["delta"], ydir=o["ydir"], y=o["y"], pre=o["pre"], g=o["g"], dxz=o["dxz"], dx_dbl=o["dx_dbl"], dWdt=o["dWdt"],
                   ckpt=o["ckpt"], dconv_w=o["cb"][1], dconv_b=o["cb"][2])
        for i, name in enumerate(("du", "ddelta", "dz", "dB", "dC", "dA", "dD", "dbias")):
            if o["sb"][i] is not None:
                res[name] = o["sb"][i]
        return res

    for k in (0, 1):
        a, b = flat(ref[k]), flat(got[k])
        for name in a:
            assert torch.equal(a[name], b[name]), (k, name)
    # the forward is really the small-launch family and every kernel of the pair shared its launch
    assert sum(c_got.values()) * 2 == sum(c_ref.values()), (c_got, c_ref)
    assert all(c_got[n] * 2 == c_ref[n] for n in c_ref), (c_got, c_ref)


def test_n_entry_points_run_incongruent_launches_one_by_one(gpu):
    """dm_*_n with structs that differ in a size: not one grid, but still both results (the second launch follows the first)."""
    from diffma_amd import hip_ops

    x0 = torch.randn(3, 40, 256, device=gpu)
    x1 = torch.randn(5, 40, 256, device=gpu)
    a, b = hip_ops.both(lambda k: hip_ops.colsum((x0, x1)[k].view(-1, 256)))
    torch.cuda.synchronize()
    torch.testing.assert_close(a, x0.view(-1, 256).sum(0), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(b, x1.view(-1, 256).sum(0), rtol=1e-5, atol=1e-4)


def test_dtproj_n_entries_check_every_struct_like_a_single_call(gpu):
    """dm_dtproj_softplus_fwd_n / dm_dtproj_bwd_n through the raw C ABI with two structs that are congruent in every size and stride,
    one of them with `xdbl` (forward) / `ddelta` (backward) starting 8 bytes into a 16-byte aligned buffer.  The kernels move 16-byte
    pieces, so the single entry rejects that struct (DM_ERR_LAYOUT forward, DM_ERR_ARG backward); the `_n` entry is documented as the
    single entry on args[0], args[1], ... in order, so: aligned struct first -> that status, the first struct's outputs bit for bit
    those of a single call, the second struct's outputs untouched; misaligned struct first -> that status and nothing written."""
    import ctypes
    from diffma_amd import _lib

    lib = _lib.load()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    raw = lambda name, a: int(getattr(lib, name)(ctypes.byref(a), stream()))

    def raw_n(name, structs):
        arr = (type(structs[0]) * len(structs))(*structs)
        return int(getattr(lib, name)(ctypes.cast(arr, ctypes.c_void_p), len(structs), stream()))

    DM_OK, DM_ERR_ARG, DM_ERR_LAYOUT, SENT = 0, -1, -2, 7.0
    dt, M, Dm, R, N = torch.bfloat16, 64, 512, 16, 16
    P, nblk = R + 2 * N, 2
    g = torch.Generator(device=gpu).manual_seed(5)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=gpu, generator=g) * sc)

    def shifted(t):
        """the same values 8 bytes into a 16-byte aligned buffer (4 spare elements on either side)"""
        buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=gpu)
        assert buf.data_ptr() % 16 == 0
        v = buf[4:4 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8
        return v

    sent = lambda *s, dtype=dt: torch.full(s, SENT, dtype=dtype, device=gpu)
    untouched = lambda *ts: all(bool((t == SENT).all()) for t in ts)

    # ---- forward: delta = softplus(xdbl[:, :R] @ w^T + bias)
    def fwd_args(xdbl, w, bias, delta):
        a = _lib.dm_dtproj_args()
        a.rows, a.dim, a.rank, a.io_dtype = M, Dm, R, _lib.DM_BF16
        a.xdbl, a.w, a.bias, a.delta, a.xd_sr = xdbl.data_ptr(), w.data_ptr(), bias.data_ptr(), delta.data_ptr(), xdbl.stride(0)
        return a

    x = [rnd(M, P).to(dt), shifted(rnd(M, P).to(dt))]
    w = [rnd(Dm, R, sc=0.3).to(dt) for _ in range(2)]
    bias = [rnd(Dm, sc=0.5) for _ in range(2)]
    ref = sent(M, Dm)
    assert raw("dm_dtproj_softplus_fwd", fwd_args(x[0], w[0], bias[0], ref)) == DM_OK
    lone = sent(M, Dm)
    assert raw("dm_dtproj_softplus_fwd", fwd_args(x[1], w[1], bias[1], lone)) == DM_ERR_LAYOUT
    for order in ((0, 1), (1, 0)):
        out = [sent(M, Dm), sent(M, Dm)]
        rc = raw_n("dm_dtproj_softplus_fwd_n", [fwd_args(x[k], w[k], bias[k], out[k]) for k in order])
        torch.cuda.synchronize()
        assert rc == DM_ERR_LAYOUT, (order, rc)
        assert untouched(out[1], lone), order
        if order == (0, 1):
            assert torch.equal(out[0], ref)
        else:
            assert untouched(out[0])

    # ---- backward: dxdbl[:, :R] = ddelta @ w, part[blk] = the workgroup's share of ddelta^T @ xdbl[:, :R]
    def bwd_args(ddelta, xdbl, w, dxdbl, part):
        a = _lib.dm_dtproj_bwd_args()
        a.rows, a.dim, a.rank, a.io_dtype, a.nblk = M, Dm, R, _lib.DM_BF16, nblk
        a.ddelta, a.xdbl, a.w, a.dxdbl, a.part = ddelta.data_ptr(), xdbl.data_ptr(), w.data_ptr(), dxdbl.data_ptr(), part.data_ptr()
        a.xd_sr, a.dxd_sr = xdbl.stride(0), dxdbl.stride(0)
        return a

    assert lib.dm_dtproj_bwd_supported(Dm, R, _lib.DM_BF16)
    dd = [rnd(M, Dm, sc=0.5).to(dt), shifted(rnd(M, Dm, sc=0.5).to(dt))]
    xb = [rnd(M, P).to(dt) for _ in range(2)]
    ref_dx, ref_part = sent(M, P), sent(nblk, Dm * R, dtype=torch.float32)
    assert raw("dm_dtproj_bwd", bwd_args(dd[0], xb[0], w[0], ref_dx, ref_part)) == DM_OK
    lone_dx, lone_part = sent(M, P), sent(nblk, Dm * R, dtype=torch.float32)
    assert raw("dm_dtproj_bwd", bwd_args(dd[1], xb[1], w[1], lone_dx, lone_part)) == DM_ERR_ARG
    for order in ((0, 1), (1, 0)):
        dx = [sent(M, P), sent(M, P)]
        part = [sent(nblk, Dm * R, dtype=torch.float32) for _ in range(2)]
        rc = raw_n("dm_dtproj_bwd_n", [bwd_args(dd[k], xb[k], w[k], dx[k], part[k]) for k in order])
        torch.cuda.synchronize()
        assert rc == DM_ERR_ARG, (order, rc)
        assert untouched(dx[1], part[1], lone_dx, lone_part), order
        if order == (0, 1):
            assert torch.equal(dx[0], ref_dx) and torch.equal(part[0], ref_part)
        else:
            assert untouched(dx[0], part[0])


# ---- dm_gemm: the projections' dense products in the small-launch regime (csrc/gemm.hip) -------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M", [196, 1568, 200, 4704])
def test_gemm_matches_fp64_matmul(gpu, dtype, M):
    """The three products of a Linear layer at the mixer's real widths (in_proj 512 -> 2048, out_proj 1024 -> 512, x_proj 1024 -> 64)
    and a ragged row count, against fp64 matmul of the same 16-bit operands: forward, input gradient, weight gradient (fp32 out),
    and the accumulating form; rel-L2 <= 1e-2 (bf16) / 2e-3 (fp16) for 16-bit results, 1e-5 for fp32 results."""
    from diffma_amd import hip_ops

    g = torch.Generator(device=gpu).manual_seed(M)
    mk = lambda *s: (torch.randn(*s, device=gpu, generator=g)).to(dtype)
    tol16 = 1e-2 if dtype == torch.bfloat16 else 2e-3
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    for K, N in ((512, 2048), (1024, 512), (1024, 64)):
        x, W, dy = mk(M, K), mk(N, K) * K ** -0.5, mk(M, N)
        assert hip_ops.gemm_supported(x, W, True, True) and hip_ops.gemm_supported(dy, W, True, False)
        y = hip_ops.gemm(x, W)                                                   # y = x W^T
        assert rel(y, x.double() @ W.double().t()) <= tol16
        dx = hip_ops.gemm(dy, W, True, False)                                    # dx = dy W
        assert rel(dx, dy.double() @ W.double()) <= tol16
        dW = hip_ops.gemm(dy, x, False, False, out_dtype=torch.float32)          # dW = dy^T x
        assert dW.dtype == torch.float32 and rel(dW, dy.double().t() @ x.double()) <= 1e-5
        acc = mk(M, K)
        want = acc.double() + dy.double() @ W.double()
        hip_ops.gemm(dy, W, True, False, out=acc, accumulate=True)               # acc += dy W
        assert rel(acc, want) <= tol16
        # strided operands: a column block of a wider buffer (the x half of xz, the dt columns of x_dbl)
        wide = mk(M, 2 * K)
        yv = hip_ops.gemm(wide[:, K:], W)
        assert rel(yv, wide[:, K:].double() @ W.double().t()) <= tol16
    torch.cuda.synchronize()


def test_gemm_pair_is_bit_identical_to_two_launches(gpu):
    from diffma_amd import _lib, hip_ops

    g = torch.Generator(device=gpu).manual_seed(5)
    mk = lambda *s: torch.randn(*s, device=gpu, generator=g).bfloat16()
    x, W, dy = [mk(392, 512), mk(392, 512)], [mk(2048, 512), mk(2048, 512)], [mk(392, 2048), mk(392, 2048)]
    ref = [(hip_ops.gemm(x[k], W[k]), hip_ops.gemm(dy[k], W[k], True, False), hip_ops.gemm(dy[k], x[k], False, False, out_dtype=torch.float32)) for k in (0, 1)]
    calls = []
    real = _lib.call_n
    _lib.call_n = lambda name, arr, st: (calls.append(name), real(name, arr, st))[1]
    try:
        got = hip_ops.both(lambda k: (hip_ops.gemm(x[k], W[k]), hip_ops.gemm(dy[k], W[k], True, False), hip_ops.gemm(dy[k], x[k], False, False, out_dtype=torch.float32)))
    finally:
        _lib.call_n = real
    torch.cuda.synchronize()
    assert calls == ["dm_gemm"] * 3
    for k in (0, 1):
        for a, b in zip(ref[k], got[k]):
            assert torch.equal(a, b)


# ---- K12: the persistent large-batch projection kernel (csrc/gemm_large.hip; reference block/mamba.py:261,315,333-337) ----------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", [(100352, 2048, 512),      # in_proj forward at the bench batch: 392 row blocks x 8 = 12.25 rounds -> 12 + K11 tail
                                   (100352, 512, 1024),       # out_proj forward: 3.06 rounds -> 3 + tail
                                   (100352, 1024, 512),       # out_proj input gradient (transposed weight copy)
                                   (100352, 512, 2048),       # in_proj input gradient
                                   (34496, 2048, 512),        # batch 176 (the end-to-end test's size): 135 row blocks -> 128 + 7
                                   (34419, 1024, 1024),       # ragged: the last row block has 115 rows (masked by the descriptors)
                                   (2048, 256, 512)])         # the smallest it takes: 8 tiles, most workgroups idle
def test_gemm_large_matches_fp64_matmul(gpu, dtype, M, N, K):
    """C = A B^T by dm_gemm_large against the fp64 product of the same 16-bit operands (computed on the device: the fp64 library
    GEMM is the checker here), every element of C: rel-L2 <= 1e-2 (bf16) / 2e-3 (fp16), and max |error| within 4 output ulps of
    the largest entry (catches a single wrong tile, which a norm over 2 x 10^8 elements would not).  Then the same product with
    strided operands -- A the x half of a wider row, C a column block of a wider buffer whose other columns must stay untouched."""
    from diffma_amd import hip_ops

    g = torch.Generator(device=gpu).manual_seed(M + N + K)
    a = (torch.rand(M, K, device=gpu, generator=g) * 2 - 1).to(dtype)
    b = ((torch.rand(N, K, device=gpu, generator=g) * 2 - 1) * K ** -0.5).to(dtype)
    assert hip_ops.gemm_large_supported(a, b)
    c = hip_ops.gemm_large(a, b)
    ref = torch.empty(M, N, dtype=torch.float64, device=gpu)
    for r0 in range(0, M, 16384):                                    # (fp64 temporaries of 16 k rows at a time)
        ref[r0:r0 + 16384] = a[r0:r0 + 16384].double() @ b.double().t()
    tol, ulp = (1e-2, 2.0 ** -8) if dtype == torch.bfloat16 else (2e-3, 2.0 ** -11)
    err = (c.double() - ref)
    assert float(err.norm() / ref.norm()) <= tol
    assert float(err.abs().max()) <= 4 * ulp * float(ref.abs().max()), float(err.abs().max())
    del err
    # strided: A = columns [K, 2K) of a [M, 2K] buffer; C = columns [N, 2N) of a [M, 3N] buffer prefilled with a marker
    wide = torch.empty(M, 2 * K, dtype=dtype, device=gpu)
    wide[:, K:] = a
    wide[:, :K] = 7.0
    cbuf = torch.full((M, 3 * N), 5.0, dtype=dtype, device=gpu)
    out = cbuf[:, N:2 * N]
    assert hip_ops.gemm_large_supported(wide[:, K:], b, out)
    hip_ops.gemm_large(wide[:, K:], b, out)
    torch.cuda.synchronize()
    assert torch.equal(out, c)
    assert float((cbuf[:, :N] - 5.0).abs().max()) == 0.0 and float((cbuf[:, 2 * N:] - 5.0).abs().max()) == 0.0


def test_gemm_large_rejects_what_it_does_not_take(gpu):
    """The predicate and the C entry agree: shapes outside the kernel's domain are refused with a status code, not launched."""
    from diffma_amd import _lib, hip_ops

    mk = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=gpu)
    assert not hip_ops.gemm_large_supported(mk(1024, 512), mk(2048, 512))        # fewer than 2048 rows
    assert not hip_ops.gemm_large_supported(mk(4096, 512), mk(320, 512))         # columns not a multiple of 256
    assert not hip_ops.gemm_large_supported(mk(4096, 384), mk(512, 384))         # contraction not a multiple of 512
    assert not hip_ops.gemm_large_supported(mk(4096, 512).float(), mk(512, 512).float())
    with pytest.raises(_lib.DiffmaHipError):
        hip_ops.gemm_large(mk(4096, 384), mk(512, 384))


@pytest.mark.parametrize("cols", [1024, 512])
def test_linear_splitk_takes_the_large_kernel_and_matches_autograd(gpu, monkeypatch, cols):
    """linear_splitk at the bench's row count: the forward and the input gradient run on K12 (the latter through the transposed
    weight copy), the weight gradient on the split-K product -- all three against fp64 autograd of the same 16-bit operands."""
    from diffma_amd import _lib
    from diffma_amd import projections as proj

    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda n, a, st: (names.append(n), real(n, a, st))[1])
    g = torch.Generator(device=gpu).manual_seed(3)
    M = 16384
    # the default policy of projections.route (outputs of 1024 columns and more): in_proj forward and out_proj input
    # gradient on K12, the two 512-column products on the library's NT kernels; with DIFFMA_GEMM_LARGE_MIN_COLS=512 all but the
    # in_proj input gradient (contraction 2048)
    monkeypatch.setattr(proj, "LARGE_MIN_COLS", cols)
    for K, N, want in ((512, 2048, 1), (1024, 512, 1 if cols == 1024 else 2)):
        x = (torch.randn(M, K, device=gpu, generator=g)).bfloat16().requires_grad_(True)
        W = (torch.randn(N, K, device=gpu, generator=g) * K ** -0.5).requires_grad_(True)       # fp32 master
        dy = torch.randn(M, N, device=gpu, generator=g).bfloat16()
        names.clear()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = proj.linear_splitk(x, W)
        y.backward(dy)
        assert names.count("dm_gemm_large") == want, names
        x64, W64 = x.detach().double().requires_grad_(True), W.detach().bfloat16().double().requires_grad_(True)
        y64 = x64 @ W64.t()
        y64.backward(dy.double())
        assert rel_l2(y.detach(), y64.detach()) <= 1e-2
        assert rel_l2(x.grad, x64.grad) <= 1e-2
        assert rel_l2(W.grad, W64.grad) <= 1e-2


# ---- K13 dm_repack: the operator boundary's layout change (channel-major (B, D, L) <-> token-major [B, L, D]) -- a move of words, bit-exact ----
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("Bsz,Dm,L,how", [
    (3, 2048, 196, "crossscan"),      # the reference's call: slice k of a contiguous (B, 3, 2 Din, L) buffer (block/mamba.py:346-348): 8-byte runs along L
    (2, 256, 64, "contiguous"),       # L % 8 == 0: 16-byte runs on both sides
    (2, 200, 49, "contiguous"),       # odd L: element accesses along L, ragged channel tile (200 = 3 x 64 + 8)
    (1, 100, 300, "contiguous"),      # two position tiles (256 + 44); dim % 8 != 0 -> element accesses on the token-major side
    (2, 64, 7, "offset"),             # misaligned base pointer on the channel-major side
    (1, 1, 1, "contiguous"),
    (2, 130, 513, "padded"),          # three position tiles, padded rows on both sides
])
def test_repack_both_directions_bit_exact(gpu, dtype, Bsz, Dm, L, how):
    from diffma_amd import hip_ops

    g = torch.Generator().manual_seed(Bsz * 1000 + Dm + L)
    if how == "crossscan":
        base = torch.randn(Bsz, 3, Dm, L, generator=g).to(dtype).to(gpu)
        cm = base[:, 1]
    elif how == "offset":
        base = torch.randn(Bsz * Dm * L + 3, generator=g).to(dtype).to(gpu)
        cm = base[3:].view(Bsz, Dm, L)
    elif how == "padded":
        base = torch.randn(Bsz, Dm + 2, L + 5, generator=g).to(dtype).to(gpu)
        cm = base[:, 1:Dm + 1, :L]
    else:
        cm = torch.randn(Bsz, Dm, L, generator=g).to(dtype).to(gpu)
    tm = hip_ops.repack(cm, True)
    assert tm.shape == (Bsz, L, Dm) and tm.is_contiguous()
    assert torch.equal(tm, cm.transpose(1, 2).contiguous())
    # and back, into a padded token-major source / strided channel-major destination
    tsrc = torch.zeros(Bsz, L, Dm + (8 if how == "padded" else 0), dtype=dtype, device=gpu)[:, :, :Dm]
    tsrc.copy_(tm)
    back = hip_ops.repack(tsrc, False)
    assert back.shape == (Bsz, Dm, L) and back.is_contiguous()
    assert torch.equal(back, cm)
    if how == "crossscan":             # written in place into a slice of the reference's (B, 3, C, L) buffer; the neighbours stay untouched
        dst = torch.full((Bsz, 3, Dm, L), 7.0, dtype=dtype, device=gpu)
        hip_ops.repack(tm, False, out=dst[:, 2])
        assert torch.equal(dst[:, 2], cm) and bool((dst[:, :2] == 7.0).all())


def test_repack_full_size_checksum(gpu):
    """BASELINE size (batch 512 x 2048 channels x 196 tokens, bf16): a transpose is a permutation of words -- the sorted multiset of a
    sample's words and per-channel sums survive it, and there-and-back is the identity."""
    from diffma_amd import hip_ops

    Bsz, Dm, L = 512, 2048, 196
    xs = torch.empty(Bsz, 3, Dm, L, dtype=torch.bfloat16, device=gpu).normal_()
    cm = xs[:, 2]
    tm = hip_ops.repack(cm, True)
    assert torch.equal(tm.view(torch.int16).sum(1, dtype=torch.int64), cm.view(torch.int16).sum(2, dtype=torch.int64))   # per (sample, channel) word sums, exact in int64
    assert torch.equal(tm[17].reshape(-1).view(torch.int16).sort().values, cm[17].reshape(-1).view(torch.int16).sort().values)
    assert torch.equal(hip_ops.repack(tm, False), cm)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mamba_inner_fn_on_crossscan_slices_hands_back_channel_major_gradients(gpu, dtype):
    """The reference's call pattern (block/mamba.py:343-348): three strided (B, 2 Din, L) slices of one buffer.  The operator's
    result equals the one on a token-major copy (the layout change moves words), and the gradient arrives CONTIGUOUS in the
    reference's layout (what CrossScan.backward and the in_proj products go on with)."""
    from diffma_amd.selective_scan_interface import mamba_inner_fn

    Bsz, Din, L, N, R, dmodel = 2, 128, 49, 16, 8, 64
    g = torch.Generator().manual_seed(5)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(gpu)
    xs = mk(Bsz, 3, 2 * Din, L).to(dtype).requires_grad_(True)
    cw, cb = mk(Din, 1, 4, sc=0.5), mk(Din, sc=0.1)
    xw, dtw, ow = mk(R + 2 * N, Din, sc=0.1), mk(Din, R, sc=0.3), mk(dmodel, Din, sc=0.1)
    A, Dp, dtb = -(torch.rand(Din, N, generator=g) * 2 + 0.2).to(gpu), mk(Din), mk(Din, sc=0.3)
    cast = (lambda t: t.to(dtype))
    args = (cast(cw), cast(cb), cast(xw), cast(dtw), cast(ow), None, A, None, None, Dp)
    outs = [mamba_inner_fn(xs[:, k], *args, delta_bias=dtb, delta_softplus=True) for k in range(3)]
    go = mk(Bsz, L, dmodel).to(dtype)
    (gx,) = torch.autograd.grad(outs, xs, [go, go * 0.5, go * 0.25])
    # the same operator on token-major copies (transposed VIEWS: no repack on this path)
    xt = xs.detach().permute(0, 1, 3, 2).contiguous().requires_grad_(True)          # (B, 3, L, 2 Din)
    outs2 = [mamba_inner_fn(xt[:, k].transpose(1, 2), *args, delta_bias=dtb, delta_softplus=True) for k in range(3)]
    (gt,) = torch.autograd.grad(outs2, xt, [go, go * 0.5, go * 0.25])
    for a, b in zip(outs, outs2):
        assert torch.equal(a, b)
    assert torch.equal(gx, gt.permute(0, 1, 3, 2))


# ---- K14 dm_adamw_ema_step: AdamW + EMA in one pass, on a torch.optim.AdamW instance's own state ----
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adamw_ema_matches_torch(gpu, wd):
    """Reference step: train.py:153-166, 259-264 (AdamW lr 1e-4 wd 0, then update_ema).  Against torch's fused AdamW followed by
    _foreach_lerp_ on identical copies: weights, both moments, the per-tensor step counters and the EMA after every one of 4 steps --
    one of them dropped through found_inf (weights / moments / counters untouched, the EMA takes its step towards the unchanged
    weights) -- for tensors of 1 element to several chunks, sizes that are not multiples of 4, and a misaligned view.  fp32 arithmetic
    with the scalars in double as torch keeps them; bound: 8 ulp, and 5e-9 absolute on the weights (2 ulp of the lr-sized update a weight near zero is the difference of)."""
    from diffma_amd import optim

    g = torch.Generator().manual_seed(7)
    shapes = [(1,), (3,), (5, 7), (1024,), (4097,), (64, 513), (3, 16384 + 1), (512, 2048)]
    base = [torch.randn(*s, generator=g).to(gpu) for s in shapes]
    odd = torch.randn(1031, generator=g).to(gpu)
    def make():
        ps = [torch.nn.Parameter(b.clone()) for b in base] + [torch.nn.Parameter(odd.clone()[1:1030])]
        return ps
    pa, pb = make(), make()
    assert pa[-1].data_ptr() % 16 != 0
    ea, eb = [p.detach().clone() * 0.5 for p in pa], [p.detach().clone() * 0.5 for p in pb]
    kw = dict(lr=1e-2, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)
    oa = torch.optim.AdamW(pa, fused=True, capturable=True, **kw)
    ob = torch.optim.AdamW(pb, fused=True, capturable=True, **kw)
    assert optim.supported(ob, pb, eb)
    fused = optim.FusedAdamWEMA(ob, pb, eb, ema_decay=0.9, ema_on_skip=True)
    for step in range(4):
        grads = [torch.randn(p.shape, generator=g).to(gpu) * (10.0 ** (step - 2)) for p in pa]
        skip = step == 2
        found = torch.full((), 1.0 if skip else 0.0, device=gpu)
        for p, q, gr in zip(pa, pb, grads):
            p.grad, q.grad = gr.clone(), (gr.clone() if not skip else torch.full_like(gr, float("nan")))
        if not skip:
            oa.step()
        torch._foreach_lerp_(ea, [p.detach() for p in pa], 1.0 - 0.9)
        fused.step(found)
        torch.cuda.synchronize()
        for i, (p, q) in enumerate(zip(pa, pb)):
            sa, sb = oa.state[p], ob.state[q]
            if len(sa) == 0:                      # torch has not stepped yet (first step skipped is not the case here)
                continue
            assert float(sa["step"]) == float(sb["step"]), (step, i)
            torch.testing.assert_close(q.detach(), p.detach(), rtol=1e-6, atol=5e-9, msg=lambda m, i=i: f"step {step} weight {i}: {m}")
            torch.testing.assert_close(sb["exp_avg"], sa["exp_avg"], rtol=1e-6, atol=1e-12, msg=lambda m, i=i: f"step {step} exp_avg {i}: {m}")
            torch.testing.assert_close(sb["exp_avg_sq"], sa["exp_avg_sq"], rtol=1e-6, atol=1e-12, msg=lambda m, i=i: f"step {step} exp_avg_sq {i}: {m}")
            torch.testing.assert_close(eb[i], ea[i], rtol=1e-6, atol=5e-9, msg=lambda m, i=i: f"step {step} ema {i}: {m}")
    assert float(oa.state[pa[0]]["step"]) == 3.0
    # the state is the optimizer's own: torch's step continues from it
    sd = ob.state_dict()
    assert len(sd["state"]) == len(pb) and float(sd["state"][0]["step"]) == 3.0


# ---- K15 against numbers the REFERENCE produced (G3: the reference's own training_losses / q_sample on a fixed fake denoiser) ----
@pytest.mark.parametrize("tag,spec", [("full", ""), ("s250", "250")])
def test_fused_training_losses_match_reference_golden(gpu, tag, spec):
    """dm_q_sample + dm_training_loss (csrc/diffusion_loss.hip) through GaussianDiffusion.training_losses on the device against
    tests/golden/g3_diffusion_steps.npz -- x_t, mse, vb and loss as the reference's gaussian_diffusion.py:715-789 computed them
    (tools/gen_golden.py ran the reference with the same deterministic stand-in denoiser): the fused path held to reference-held
    values, not to this repository's generic path.  fp32: rtol 2e-5 like the CPU test of the generic path."""
    import numpy as np
    from diffma_amd.diffusion import create_diffusion

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g3_diffusion_steps.npz"))
    x0, noise = (torch.from_numpy(g[k]).to(gpu) for k in ("x0", "noise"))
    t = torch.from_numpy(g[f"{tag}.t"]).to(gpu)
    d = create_diffusion(spec)
    seen = {}

    def fake_model(x, tt, **kw):                       # tools/gen_golden.py fake_model
        seen["x_t"] = x
        return torch.cat([torch.sin(x) + tt.view(-1, 1, 1, 1).float() / 1000.0, torch.cos(x)], dim=1)

    from diffma_amd import _lib
    log = []
    real_call = _lib.call
    _lib.call = lambda name, a, st: (log.append(name), real_call(name, a, st))[1]
    try:
        assert d.fused_loss
        terms = d.training_losses(fake_model, x0, t, noise=noise)
    finally:
        _lib.call = real_call
    assert "dm_q_sample" in log and "dm_training_loss" in log, log     # the fused kernels are what ran
    np.testing.assert_allclose(seen["x_t"].cpu().numpy(), g[f"{tag}.q_sample"], rtol=2e-5, atol=2e-6)
    for k in ("mse", "vb", "loss"):
        np.testing.assert_allclose(terms[k].detach().cpu().numpy(), g[f"{tag}.loss.{k}"], rtol=2e-5, atol=2e-6, err_msg=f"{tag}.loss.{k}")


# ---- K15 dm_q_sample / dm_training_loss: the diffusion wrapper around the denoiser call of a training step ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("spec", ["", "250"])
def test_fused_training_losses_match_the_generic_path(gpu, dtype, spec):
    """GaussianDiffusion.training_losses (reference gaussian_diffusion.py:715-789) for the training configuration: q_sample + mse + the
    variational-bound term (KL rows and, at t = 0, the discretised decoder NLL with all three branches of its `where`: x_0 < -0.999,
    > 0.999, between) + their gradients with respect to the model output -- the two-launch path against the ATen chain on the same
    inputs (fp32 and 16-bit model outputs: the reference's expression rounds (v + 1) / 2 in the output's dtype), full and respaced
    schedules, and against autograd for each of the three returned terms separately."""
    from diffma_amd.diffusion import create_diffusion

    d = create_diffusion(spec)
    B, C, H = 12, 4, 28
    g = torch.Generator().manual_seed(41)
    x0 = torch.randn(B, C, H, H, generator=g).clamp(-1.2, 1.2)
    x0[0, 0, 0, :8] = torch.tensor([-1.0, -0.9995, 0.9995, 1.0, 0.999, -0.999, 0.5, 1.2])
    x0[1] = x0[0]
    nz = torch.randn(B, C, H, H, generator=g)
    t = torch.randint(0, d.num_timesteps, (B,), generator=g)
    t[0], t[1], t[2], t[3] = 0, 1, 0, d.num_timesteps - 1
    leaf0 = torch.randn(B, 2 * C, H, H, generator=g)
    leaf0[:, C:] = leaf0[:, C:].clamp(-1.5, 1.5)
    x0, nz, t = x0.to(gpu), nz.to(gpu), t.to(gpu)

    def run(fused, which, upcast=False):
        d.fused_loss = fused
        leaf = leaf0.to(gpu).requires_grad_(True)
        seen = {}
        def model(x_t, tt, **kw):
            seen["x_t"] = x_t
            return leaf.to(dtype).float() if upcast else leaf.to(dtype)
        terms = d.training_losses(model, x0, t, noise=nz)
        w = torch.linspace(0.5, 1.5, B, device=gpu)
        (terms[which] * w).sum().backward()
        return {k: v.detach() for k, v in terms.items()}, leaf.grad.detach(), seen["x_t"].detach()

    try:
        for which in ("loss", "mse", "vb"):
            ref, gref, xt_ref = run(False, which)
            got, ggot, xt_got = run(True, which)
            torch.testing.assert_close(xt_got, xt_ref, rtol=1e-6, atol=1e-6)
            for k in ("mse", "vb", "loss"):
                torch.testing.assert_close(got[k], ref[k], rtol=2e-5, atol=1e-6, msg=lambda m, k=k: f"{which}/{k}: {m}")
            assert float(gref.abs().max()) > 0
            if dtype == torch.float32:
                torch.testing.assert_close(ggot, gref, rtol=2e-4, atol=2e-6 * float(gref.abs().max()), msg=lambda m: f"grad for {which}: {m}")
            else:
                # The ATen chain on a 16-bit output rounds every intermediate gradient to 16 bits -- d logvar / d frac reaches v as the
                # DIFFERENCE of two rounded products g * log(beta_t) - g * log(posterior_var_t), which cancel to a few per cent of either:
                # its v-gradient is noise at the 4 % level (measured).  The yardstick for the gradient is therefore the same chain on
                # the fp32 UPCAST of the same rounded output; the kernel rounds once, at the end.
                _, gref, _ = run(False, which, upcast=True)
                # (what is left against that yardstick is the reference's own rounding of (v + 1) / 2 to 16 bits, which the kernel keeps so
                #  that the VALUES agree with the reference's expression: 1 - exp(d) near d = 0 turns 2^-9 of frac into 1-2 % of the gradient)
                assert rel_l2(ggot, gref) <= (3e-2 if which == "vb" else 1e-2), (which, rel_l2(ggot, gref))
                off = (ggot - gref).abs() > 3e-2 * gref.abs() + 2e-2 * float(gref.abs().max())
                assert float(off.float().mean()) <= 1e-3, (which, float(off.float().mean()))
    finally:
        d.fused_loss = True
