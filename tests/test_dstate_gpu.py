"""d_state 64 and 128, from the scan kernels up to the model (the widths the reference's `d_state` config key can ask for beyond
its default of 16, and Mamba2's own default of 128).

Kernels: the helpers, tolerances and checks of tests/test_kernels_gpu.py, unchanged (TOL, the tables inside _scan_bwd_case).
Mixers and models: the bounds of the d_state-16 tests of the same thing in tests/test_model_gpu.py.  Shapes are the smallest that
reach every tail: L = 1 and 3 are shorter than a checkpoint interval, 21 is no multiple of 4 or 8, 40 is several staging chunks;
Dm = 64 is one workgroup or less, 200 a ragged last workgroup at 64 and at 32 channels per workgroup, 128 more than one.
"""
import pytest
import torch

from tests.test_kernels_gpu import TOL, _ckpt_states, _inputs, _oracle_scan, _oracle_states, _scan_bwd_case
from tests.test_model_gpu import _rerandomize, rel_l2

pytestmark = pytest.mark.gpu

WIDE = [64, 128]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
dtype_ids = lambda ds: [IDS[d] for d in ds]


# ---- K1 forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids(DTYPES))
@pytest.mark.parametrize("N", WIDE)
@pytest.mark.parametrize("S,L,Dm", [(2, 21, 64), (1, 3, 200), (2, 1, 64), (2, 40, 128)])
def test_scan_fwd_wide_matches_oracle(gpu, dtype, N, S, L, Dm):
    from diffma_amd import hip_ops

    host, d = _inputs(S, L, Dm, N, dtype, seed=L * 7 + Dm + N, dev=gpu)
    last = torch.empty(S, N, Dm, device=gpu)
    out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["bias"], True, last_state=last)
    torch.cuda.synchronize()
    ref, ref_last = _oracle_scan(host)
    rtol, atol = TOL[dtype]
    torch.testing.assert_close(out.float().cpu().double(), ref, rtol=rtol, atol=atol * max(1.0, ref.abs().max().item()))
    torch.testing.assert_close(last.cpu().double().permute(0, 2, 1), ref_last, rtol=1e-4, atol=1e-5 * max(1.0, ref_last.abs().max().item()))


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids(DTYPES))
@pytest.mark.parametrize("N", WIDE)
def test_scan_fwd_wide_row_index_and_checkpoints(gpu, dtype, N):
    """3 directions over a batch of 2 sharing one z through the row tables, with last_state, and EVERY checkpoint slot against the
    fp64 state (fp32 rows for fp32 / fp16 I/O, packed bf16 pairs for bf16 I/O), at the bounds
    test_scan_fwd_chunk_parallel_long_memory states for the two formats."""
    from diffma_amd import hip_ops
    from oracle.mamba_ref import selective_scan_ref

    Bsz, ndir, L, Dm = 2, 3, 21, 200
    S = Bsz * ndir
    host, d = _inputs(S, L, Dm, N, dtype, seed=11 + N, dev=gpu, with_z=False)
    g = torch.Generator().manual_seed(3)
    zsrc = torch.randn(Bsz, L, Dm, generator=g).to(dtype)
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).int()
    operms = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)]).int()
    K = hip_ops.SCAN_CKPT_EVERY
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dtype, gpu).zero_()
    last = torch.empty(S, N, Dm, device=gpu)
    out = hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], zsrc.to(gpu), d["bias"], True, z_row_index=perms.to(gpu),
                           out_row_index=operms.to(gpu), batch_per_dir=Bsz, ckpt=ckpt, ckpt_every=K, last_state=last)
    torch.cuda.synchronize()
    out = out.float().cpu()
    got_h = _ckpt_states(ckpt, N, Dm).cpu().double()
    rtol, atol = TOL[dtype]
    for s in range(S):
        k, b = divmod(s, Bsz)
        cm = lambda t: t[s:s + 1].float().permute(0, 2, 1).double()
        zz = zsrc[b][perms[k].long()].float().T[None].double()
        ref, ref_last = selective_scan_ref(cm(host["u"]), cm(host["delta"]), host["A"].double(), cm(host["B"]), cm(host["C"]), host["D"].double(),
                                           z=zz, delta_bias=host["bias"].double(), delta_softplus=True, return_last_state=True)
        torch.testing.assert_close(out[s][operms[k].long()].double(), ref[0].T, rtol=rtol, atol=atol * max(1.0, ref.abs().max().item()))
        torch.testing.assert_close(last[s].cpu().double().T, ref_last[0], rtol=1e-4, atol=1e-5 * max(1.0, ref_last.abs().max().item()))
        hs = _oracle_states(host, s)
        for c in range(hip_ops.scan_nchunk(L, K)):
            want = hs[(c * K if c else L) - 1].T                                                    # [N, Dm]
            tol32 = 1e-4 * want.abs() + 1e-5 * max(1.0, float(want.abs().max()))
            tol = tol32 if ckpt.dtype != torch.int32 else 2.0 ** -8 * want.abs() + (1 + 2.0 ** -8) * tol32
            err = (got_h[s, c] - want).abs()
            assert bool((err <= tol).all()), (s, c, float((err / tol).max()))


# ---- K2 backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids(DTYPES))
@pytest.mark.parametrize("N", WIDE)
@pytest.mark.parametrize("S,L,Dm,kw", [
    (2, 21, 128, dict()),
    (4, 40, 200, dict(indexed=True, Bsz=2)),
    (2, 3, 64, dict()),
    (2, 1, 64, dict()),
    (2, 40, 128, dict(long_memory=True)),
    (2, 21, 128, dict(delta_softplus=False)),
], ids=["21x128", "40x200-indexed", "3x64", "1x64", "40x128-long-memory", "21x128-no-softplus"])
def test_scan_bwd_wide_matches_oracle_autograd(gpu, dtype, N, S, L, Dm, kw):
    _scan_bwd_case(gpu, dtype, S, L, Dm, N, seed=N + L + Dm, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", WIDE)
def test_scan_bwd_wide_fp32_bc(gpu, dtype, N):
    _scan_bwd_case(gpu, dtype, 4, 40, 200, N, seed=N + 3, indexed=True, Bsz=2, bc_fp32=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", WIDE)
@pytest.mark.parametrize("S,L,Dm,Bsz", [(3, 40, 128, 1), (6, 21, 256, 2)])
def test_scan_bwd_wide_mamba2_call_pattern(gpu, dtype, N, S, L, Dm, Bsz):
    """One decay per channel (DM_FLAG_A_SHARED: the one-exp instantiations) with per-direction gradients (DM_FLAG_DOUT_PER_SEQ)."""
    _scan_bwd_case(gpu, dtype, S, L, Dm, N, seed=N + L, indexed=True, Bsz=Bsz, a_shared=True, dout_per_seq=True, long_memory=True)


# ---- operators -----------------------------------------------------------------------------------------------------------------
def test_selective_scan_fn_d_state_64(gpu):
    """The reference's channel-major signature with return_last_state, forward and backward against selective_scan_ref autograd
    (bounds of test_reference_operator_signatures)."""
    from diffma_amd.selective_scan_interface import selective_scan_fn
    from oracle.mamba_ref import selective_scan_ref

    gen = torch.Generator().manual_seed(64)
    B, Din, L, N = 2, 64, 21, 64
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc)
    u, delta, z = mk(B, Din, L), mk(B, Din, L, sc=0.5), mk(B, Din, L)
    A, Bm, Cm, Dp, bias = -(torch.rand(Din, N, generator=gen) * 3 + 0.2), mk(B, N, L), mk(B, 1, N, L), mk(Din), mk(Din, sc=0.3)
    leaves = [t.to(gpu).requires_grad_(True) for t in (u, delta, A, Bm, Cm, Dp, z, bias)]
    out, last = selective_scan_fn(*leaves[:6], z=leaves[6], delta_bias=leaves[7], delta_softplus=True, return_last_state=True)
    assert out.shape == (B, Din, L) and last.shape == (B, Din, N)
    dy = mk(B, Din, L)
    (out * dy.to(gpu)).sum().backward()
    ref_leaves = [t.double().requires_grad_(True) for t in (u, delta, A, Bm, Cm, Dp, z, bias)]
    ro, rl = selective_scan_ref(*ref_leaves[:6], z=ref_leaves[6], delta_bias=ref_leaves[7], delta_softplus=True, return_last_state=True)
    (ro * dy.double()).sum().backward()
    assert rel_l2(out.detach().cpu(), ro.detach()) <= 1e-4 and rel_l2(last.cpu(), rl.detach()) <= 1e-4
    for a, b, name in zip(leaves, ref_leaves, "u delta A B C D z bias".split()):
        assert rel_l2(a.grad.cpu(), b.grad) <= 5e-4, (name, rel_l2(a.grad.cpu(), b.grad))


def test_mamba_inner_fn_d_state_64_bf16(gpu):
    """mamba_inner_fn at d_state 64, dt_rank 8, d_inner 128 in bf16 against fp64 autograd of mamba_inner_ref on the same (rounded)
    operands: forward at the operator's bf16 bound (2e-2, test_mamba_inner_fn_matches_reference_step), gradients at 3x that, as the
    mixer tests allow for theirs (_mixer_case)."""
    from diffma_amd.selective_scan_interface import mamba_inner_fn
    from oracle.mamba_ref import mamba_inner_ref

    Bsz, Din, L, N, R, dmodel = 2, 128, 21, 64, 8, 64
    dtype, tol = torch.bfloat16, 2e-2
    g = torch.Generator().manual_seed(5)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype)
    xz = mk(Bsz, 2 * Din, L)
    cw, cb = mk(Din, 1, 4, sc=0.5), mk(Din, sc=0.1)
    xw, dtw, ow = mk(R + 2 * N, Din, sc=0.1), mk(Din, R, sc=0.3), mk(dmodel, Din, sc=0.1)
    A, Dp, dtb = -(torch.rand(Din, N, generator=g) * 2 + 0.2), torch.randn(Din, generator=g), torch.randn(Din, generator=g) * 0.3
    go = torch.randn(Bsz, L, dmodel, generator=g)
    names = "xz conv_w conv_b x_proj dt_proj out_proj A D dt_bias".split()
    host = (xz, cw, cb, xw, dtw, ow, A, Dp, dtb)
    dv = [t.to(gpu).requires_grad_(True) for t in host]
    out = mamba_inner_fn(dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], None, dv[6], None, None, dv[7], delta_bias=dv[8], delta_softplus=True)
    (out.float() * go.to(gpu)).sum().backward()
    rf = [t.double().requires_grad_(True) for t in host]
    ro = mamba_inner_ref(rf[0], rf[1], rf[2], rf[3], rf[4], rf[5], None, rf[6], None, None, rf[7], delta_bias=rf[8], delta_softplus=True)
    (ro * go.double()).sum().backward()
    assert out.shape == (Bsz, L, dmodel)
    assert rel_l2(out.detach().float().cpu(), ro.detach()) <= tol, rel_l2(out.detach().float().cpu(), ro.detach())
    for name, a, b in zip(names, dv, rf):
        r = rel_l2(a.grad.float().cpu(), b.grad)
        assert r <= 3 * tol, (name, r)


# ---- mixers --------------------------------------------------------------------------------------------------------------------
def _spiral_lists(n, k):
    from diffma_amd.tools import spiral

    orders, inverses = spiral(n)
    return (orders[k], orders[k + 1], inverses[k], inverses[k + 1])


@pytest.mark.parametrize("batch", [2, 1])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d_state", WIDE)
def test_mamba_mixer_wide(gpu, d_state, dtype, tol, batch):
    """Mamba(d_model=64) on the spiral lists of a 4 x 4 grid: forward and every gradient against mamba_spiral_forward_ref in fp64,
    at the bounds of the d_state-16 mixer tests (_mixer_case: tol, 3 tol for gradients)."""
    from diffma_amd.mamba import Mamba
    from oracle.mamba_ref import mamba_spiral_forward_ref

    torch.manual_seed(d_state + batch)
    n, d_model = 4, 64
    lists = _spiral_lists(n, 2)
    mix = Mamba(d_model=d_model, d_state=d_state, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                origina_list_reversal=lists[3]).to(gpu)
    with torch.no_grad():
        mix.A_log.add_(torch.randn_like(mix.A_log) * 0.2)
        mix.D.add_(torch.randn_like(mix.D) * 0.2)
    x = torch.randn(batch, n * n, d_model, device=gpu, requires_grad=True)
    dy = torch.randn(batch, n * n, d_model, device=gpu)
    with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
        y = mix(x, "spiral")
    (y.float() * dy).sum().backward()
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mix.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    yr = mamba_spiral_forward_ref(x64, params, lists, dtype=torch.float64)
    (yr * dy.cpu().double()).sum().backward()
    assert rel_l2(y.detach().float().cpu(), yr.detach()) <= tol, rel_l2(y.detach().float().cpu(), yr.detach())
    assert rel_l2(x.grad.cpu(), x64.grad) <= 3 * tol, rel_l2(x.grad.cpu(), x64.grad)
    for k, p in mix.named_parameters():
        assert rel_l2(p.grad.cpu(), params[k].grad) <= 3 * tol, (k, rel_l2(p.grad.cpu(), params[k].grad))


@pytest.mark.parametrize("batch", [2, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d_state", [64, None], ids=["64", "default-128"])
def test_mamba2_mixer_wide(gpu, d_state, dtype, batch):
    """Mamba2(d_model=64) (headdim 64: two heads) with d_state 64 and with its own default of 128, against
    mamba2_spiral_forward_ref in fp64.  fp32: the bounds of test_mamba2_mixer_forward_backward (1e-4, 5e-4 for gradients); bf16
    autocast: those of test_mamba2_mixer_training_on_the_matrix_pipe (2e-2 / 3e-2 for dx / 4e-2 for parameters)."""
    from diffma_amd.mamba2 import Mamba2
    from oracle.mamba2_ref import mamba2_spiral_forward_ref

    torch.manual_seed(7 + batch)
    n = 4
    lists = _spiral_lists(n, 4)
    kw = {} if d_state is None else dict(d_state=d_state)
    mix = Mamba2(d_model=64, d_conv=4, expand=2, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                 origina_list_reversal=lists[3], **kw).to(gpu)
    assert mix.d_state == (128 if d_state is None else d_state) and mix.nheads == 2
    with torch.no_grad():
        mix.norm.weight.add_(torch.randn_like(mix.norm.weight) * 0.1)
        mix.D.add_(torch.randn_like(mix.D) * 0.1)
    x = torch.randn(batch, n * n, 64, device=gpu, requires_grad=True)
    dy = torch.randn(batch, n * n, 64, device=gpu)
    with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
        y = mix(x, "spiral")
    (y.float() * dy).sum().backward()
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mix.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    yr = mamba2_spiral_forward_ref(x64, params, lists, headdim=64, dtype=torch.float64)
    (yr * dy.cpu().double()).sum().backward()
    ty, tx, tp = (1e-4, 5e-4, 5e-4) if dtype == torch.float32 else (2e-2, 3e-2, 4e-2)
    assert rel_l2(y.detach().float().cpu(), yr.detach()) <= ty, rel_l2(y.detach().float().cpu(), yr.detach())
    assert rel_l2(x.grad.cpu(), x64.grad) <= tx, rel_l2(x.grad.cpu(), x64.grad)
    for k, p in mix.named_parameters():
        assert rel_l2(p.grad.float().cpu(), params[k].grad) <= tp, (k, rel_l2(p.grad.float().cpu(), params[k].grad))


# ---- the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(d_state=64), dict(use_mamba2=True, d_state=128)], ids=["mamba-64", "mamba2-128"])
def test_tiny_diffma_wide_forward_training_backward_and_graph(gpu, kw):
    """The tiny model of the d_state-16 tests at the wide states: forward against diffma_forward_ref (fp32, rel-L2 <= 1e-3), the
    training_losses backward against fp64 autograd of the oracle (loss 2e-3, every parameter gradient rel-L2 <= 5e-3:
    test_training_step_gradients_match_oracle_autograd), and one hipGraph replay of the forward equal to the eager call
    (test_graphed_denoiser_matches_eager)."""
    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.graphed import GraphedDenoiser
    from diffma_amd.model import DiffMa
    from oracle.model_ref import diffma_forward_ref

    m2 = kw.get("use_mamba2", False)
    torch.manual_seed(21)
    net = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=4, **kw)
    _rerandomize(net, 22)
    depth, L, B = len(net.blocks), 16, 2
    g = torch.Generator().manual_seed(23)
    x, y, y2 = torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 64, generator=g), torch.randn(B, L, 64, generator=g)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g))
    t = torch.tensor([437, 12])
    nz = torch.randn(B, 4, 8, 8, generator=g)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ref = diffma_forward_ref(sd, x, t, y, y2, w, patch_size=2, depth=depth, dtype=torch.float32, use_mamba2=m2)
    net = net.to(gpu).train()
    dev = lambda v: v.to(gpu)
    with torch.no_grad():
        out = net(dev(x), dev(t), y=dev(y), y2=dev(y2), w=dev(w))
    assert float(ref.abs().mean()) > 1e-3                          # a live output, not the zero-init one
    assert rel_l2(out.cpu(), ref) <= 1e-3, rel_l2(out.cpu(), ref)

    d = create_diffusion("")
    loss = d.training_losses(net, dev(x), dev(t), dict(y=dev(y), y2=dev(y2), w=dev(w)), noise=dev(nz))["loss"].mean()
    loss.backward()
    got = {k: p.grad.detach().cpu().double() for k, p in net.named_parameters() if p.grad is not None}
    sd64 = {k: v.double().clone().requires_grad_(k != "pos_embed") for k, v in sd.items()}
    model = lambda xx, tt, **kws: diffma_forward_ref(sd64, xx, tt, kws["y"], kws["y2"], kws["w"], patch_size=2, depth=depth,
                                                     dtype=torch.float64, use_mamba2=m2)
    ref_loss = d.training_losses(model, x.double(), t, dict(y=y.double(), y2=y2.double(), w=w.double()), noise=nz.double())["loss"].mean()
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 2e-3 * abs(float(ref_loss.detach()))
    for k, gr in got.items():
        r = rel_l2(gr, sd64[k].grad)
        assert r <= 5e-3, (k, r)
    assert len(got) == sum(1 for k in sd64 if k != "pos_embed")

    net.eval()
    with torch.no_grad():
        eager = net(dev(x), dev(t), y=dev(y), y2=dev(y2), w=dev(w))
    gd = GraphedDenoiser(net, dev(x), dev(t), dev(y), dev(y2), dev(w))
    torch.testing.assert_close(gd(dev(x), dev(t), y=dev(y), y2=dev(y2), w=dev(w)).clone(), eager, rtol=0, atol=0)
