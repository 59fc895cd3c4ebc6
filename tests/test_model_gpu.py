"""GPU parity of the operators (reference-facing API), the Mamba mixer, and the whole DiffMa denoiser.

End-to-end tolerances: fp32 rel-L2 <= 1e-3, bf16 autocast rel-L2 <= 2e-2 against the output
of the reference's own classes (tests/golden/g5_tiny_diffma.npz; operator = fp64 oracle stub).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _g5(gpu):
    from diffma_amd.model import DiffMa

    g = np.load(os.path.join(G, "g5_tiny_diffma.npz"))
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    net = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=4, d_state=16)
    net.load_state_dict(sd)
    net = net.to(gpu).eval()
    inp = {k: torch.from_numpy(g[k]).to(gpu) for k in ("x", "t", "y", "y2", "w")}
    return g, sd, net, inp


def test_diffma_forward_matches_reference_fp32(gpu):
    g, sd, net, inp = _g5(gpu)
    acts = {}
    hooks = [b.register_forward_hook(lambda m, i, o, k=k: acts.__setitem__(k, o.detach().cpu())) for k, b in enumerate(net.blocks)]
    with torch.no_grad():
        out = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).cpu()
    for h in hooks:
        h.remove()
    ref = torch.from_numpy(g["out"])
    assert rel_l2(out, ref) <= 1e-3, rel_l2(out, ref)
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-4)
    for k in range(4):
        assert rel_l2(acts[k], torch.from_numpy(g[f"act.block{k}"])) <= 1e-3


@pytest.mark.parametrize("depth", [9, 13])
def test_deep_diffma_forward_matches_reference(gpu, depth):
    """G12 (reference `DiffMa` class at depth 9 / 13, hidden 32): spiral lists 8..15, the wrap at block 8 (model.py:147-150)
    and the odd / deep skip pairs (model.py:286-295) on the device, output and every block activation."""
    from diffma_amd.model import DiffMa

    g = np.load(os.path.join(G, "g12_deep_tiny_diffma.npz"))
    tag = f"d{depth}"
    sd = {k[len(tag) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}.sd.")}
    net = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=32, depth=depth, d_state=16)
    net.load_state_dict(sd)
    net = net.to(gpu).eval()
    inp = {k: torch.from_numpy(g[f"{tag}.{k}"]).to(gpu) for k in ("x", "t", "y", "y2", "w")}
    acts = {}
    hooks = [b.register_forward_hook(lambda m, i, o, k=k: acts.__setitem__(k, o.detach().cpu())) for k, b in enumerate(net.blocks)]
    with torch.no_grad():
        out = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).cpu()
    for h in hooks:
        h.remove()
    ref = torch.from_numpy(g[f"{tag}.out"])
    assert rel_l2(out, ref) <= 1e-3, rel_l2(out, ref)
    for k in range(depth):
        assert rel_l2(acts[k], torch.from_numpy(g[f"{tag}.act.block{k}"])) <= 1e-3, (k, rel_l2(acts[k], torch.from_numpy(g[f"{tag}.act.block{k}"])))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).float().cpu()
    assert rel_l2(out16, ref) <= 5e-2, rel_l2(out16, ref)       # 9 / 13 blocks deep: the bf16 error of G5's 4 blocks (<= 2e-2) compounds


def test_diffma_forward_bf16_autocast(gpu):
    g, sd, net, inp = _g5(gpu)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).float().cpu()
    assert rel_l2(out, torch.from_numpy(g["out"])) <= 2e-2


def test_training_losses_match_reference(gpu):
    from diffma_amd.diffusion import create_diffusion

    g, sd, net, inp = _g5(gpu)
    d = create_diffusion("")
    z, nz, tt = (torch.from_numpy(g[k]).to(gpu) for k in ("loss_z", "loss_noise", "loss_t"))
    with torch.no_grad():
        tl = d.training_losses(net, z, tt, dict(y=inp["y"], y2=inp["y2"], w=inp["w"]), noise=nz)
    for k, v in tl.items():
        np.testing.assert_allclose(v.cpu().numpy(), g[f"loss.{k}"], rtol=2e-3, atol=1e-5, err_msg=k)


def test_training_step_gradients_match_oracle_autograd(gpu):
    """loss.backward() through the HIP autograd path == fp64 autograd through the CPU oracle model."""
    from diffma_amd.diffusion import create_diffusion
    from oracle.model_ref import diffma_forward_ref

    g, sd, net, inp = _g5(gpu)
    net.train()
    d = create_diffusion("")
    z, nz, tt = (torch.from_numpy(g[k]) for k in ("loss_z", "loss_noise", "loss_t"))
    kw = dict(y=inp["y"], y2=inp["y2"], w=inp["w"])
    loss = d.training_losses(net, z.to(gpu), tt.to(gpu), kw, noise=nz.to(gpu))["loss"].mean()
    loss.backward()
    got = {k: p.grad.detach().cpu().double() for k, p in net.named_parameters() if p.grad is not None}

    sd64 = {k: v.double().clone().requires_grad_(k != "pos_embed") for k, v in sd.items()}
    cpu_in = {k: v.cpu() for k, v in inp.items()}
    model = lambda x, t, **kws: diffma_forward_ref(sd64, x, t, kws["y"], kws["y2"], kws["w"], patch_size=2, depth=4, dtype=torch.float64)
    ref_loss = d.training_losses(model, z.double(), tt, dict(y=cpu_in["y"].double(), y2=cpu_in["y2"].double(), w=cpu_in["w"].double()),
                                 noise=nz.double())["loss"].mean()
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 2e-3 * abs(float(ref_loss.detach()))
    worst = 0.0
    for k, gr in got.items():
        ref = sd64[k].grad
        assert ref is not None, k
        r = rel_l2(gr, ref)
        worst = max(worst, r)
        assert r <= 5e-3, (k, r)
    assert len(got) == sum(1 for k in sd64 if k != "pos_embed")


def _mixer_case(gpu, dtype, tol, d_model=64, d_state=16):
    from diffma_amd.mamba import Mamba
    from diffma_amd.tools import spiral
    from oracle.mamba_ref import mamba_spiral_forward_ref

    torch.manual_seed(0)
    n = 4
    orders, inverses = spiral(n)
    lists = (orders[2], orders[3], inverses[2], inverses[3])
    mix = Mamba(d_model=d_model, d_state=d_state, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                origina_list_reversal=lists[3]).to(gpu)
    with torch.no_grad():
        mix.A_log.add_(torch.randn_like(mix.A_log) * 0.2)
        mix.D.add_(torch.randn_like(mix.D) * 0.2)
    x = torch.randn(3, n * n, d_model, device=gpu, requires_grad=True)
    dy = torch.randn(3, n * n, d_model, device=gpu)
    with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
        y = mix(x, "spiral")
    (y.float() * dy).sum().backward()
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mix.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    yr = mamba_spiral_forward_ref(x64, params, lists, dtype=torch.float64)
    (yr * dy.cpu().double()).sum().backward()
    assert rel_l2(y.detach().float().cpu(), yr.detach()) <= tol
    assert rel_l2(x.grad.cpu(), x64.grad) <= 3 * tol
    for k, p in mix.named_parameters():
        assert rel_l2(p.grad.cpu(), params[k].grad) <= 3 * tol, k


def test_mamba_mixer_forward_backward_fp32(gpu):
    _mixer_case(gpu, torch.float32, 1e-4)


def test_mamba_mixer_forward_backward_bf16(gpu):
    _mixer_case(gpu, torch.bfloat16, 2e-2)


@pytest.mark.parametrize("d_state", [8, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mamba_mixer_autocast_other_d_state(gpu, d_state, dtype):
    """`d_state` is a config key of the reference (train.py:130-135).  Under 16-bit autocast with d_model 128 (dt_rank 8,
    d_inner 256) the hoisted-softplus forward IS available, but its backward flag exists for d_state 16 only -- such a model used to
    run forward and then raise DM_ERR_ARG in backward.  The mixer must keep the softplus inside the scans for these widths and train."""
    _mixer_case(gpu, dtype, 2e-2 if dtype == torch.bfloat16 else 4e-3, d_model=128, d_state=d_state)


def test_reference_operator_signatures(gpu):
    """selective_scan_fn / mamba_inner_fn / causal_conv1d_fn with the reference's (B, D, L) layout and call
    pattern (block/mamba.py:346), including genuinely L-contiguous inputs (repack path) and autograd."""
    from diffma_amd.selective_scan_interface import causal_conv1d_fn, mamba_inner_fn, selective_scan_fn
    from oracle.mamba_ref import causal_conv1d_ref, mamba_inner_ref, selective_scan_ref

    gen = torch.Generator().manual_seed(3)
    B, Din, L, N, R, dm = 2, 128, 49, 16, 8, 64
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
        assert rel_l2(a.grad.cpu(), b.grad) <= 5e-4, name

    x = mk(B, Din, L)
    w, b = mk(Din, 4, sc=0.5), mk(Din, sc=0.1)
    y = causal_conv1d_fn(x.to(gpu), w.to(gpu), b.to(gpu), activation="silu")
    assert rel_l2(y.cpu(), causal_conv1d_ref(x.double(), w.double(), b.double(), activation="silu")) <= 1e-5
    y = causal_conv1d_fn(x.to(gpu), w.to(gpu), None, activation=None)
    assert rel_l2(y.cpu(), causal_conv1d_ref(x.double(), w.double(), None)) <= 1e-5

    xz = mk(B, 3, 2 * Din, L)[:, 1]          # a strided slice, like CrossScan hands out (block/mamba.py:346)
    cw, cb = mk(Din, 1, 4, sc=0.5), mk(Din, sc=0.1)
    xw, dw, ow = mk(R + 2 * N, Din, sc=0.1), mk(Din, R, sc=0.3), mk(dm, Din, sc=0.1)
    o = mamba_inner_fn(xz.to(gpu), cw.to(gpu), cb.to(gpu), xw.to(gpu), dw.to(gpu), ow.to(gpu), None, A.to(gpu), None, None,
                       Dp.to(gpu), delta_bias=bias.to(gpu), delta_softplus=True)
    ro = mamba_inner_ref(xz.double(), cw, cb, xw, dw, ow, None, A, None, None, Dp, delta_bias=bias, delta_softplus=True)
    assert o.shape == (B, L, dm) and rel_l2(o.cpu(), ro) <= 1e-4


def test_sampling_loops_on_device(gpu):
    from diffma_amd.diffusion import create_diffusion

    g, sd, net, inp = _g5(gpu)
    d = create_diffusion("10")
    kw = dict(y=inp["y"], y2=inp["y2"], w=inp["w"])
    torch.manual_seed(5)
    z = torch.randn(2, 4, 8, 8, device=gpu)
    torch.manual_seed(6)
    a = d.p_sample_loop(net.forward, z.shape, z, clip_denoised=False, model_kwargs=kw, device=gpu)
    torch.manual_seed(6)
    b = d.p_sample_loop(net.forward, z.shape, z, clip_denoised=False, model_kwargs=kw, device=gpu)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    c = create_diffusion("ddim50")
    s = c.ddim_sample_loop(net.forward, z.shape, z, clip_denoised=False, model_kwargs=kw, device=gpu)
    assert torch.isfinite(s).all() and s.shape == z.shape


# ---- Mamba-2 (--use-mamba2, BASELINE config 4) ---------------------------------------------------------------------------
def test_diffma_mamba2_forward_matches_reference(gpu):
    from diffma_amd.model import DiffMa

    g = np.load(os.path.join(G, "g7_tiny_diffma_mamba2.npz"))
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    net = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=4, d_state=16, use_mamba2=True)
    net.load_state_dict(sd)
    net = net.to(gpu).eval()
    inp = {k: torch.from_numpy(g[k]).to(gpu) for k in ("x", "t", "y", "y2", "w")}
    with torch.no_grad():
        out = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).cpu()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out16 = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).float().cpu()
    ref = torch.from_numpy(g["out"])
    assert rel_l2(out, ref) <= 1e-3, rel_l2(out, ref)
    assert rel_l2(out16, ref) <= 2e-2, rel_l2(out16, ref)


def test_mamba2_mixer_forward_backward(gpu):
    from diffma_amd.mamba2 import Mamba2
    from diffma_amd.tools import spiral
    from oracle.mamba2_ref import mamba2_spiral_forward_ref

    torch.manual_seed(1)
    n = 4
    orders, inverses = spiral(n)
    lists = (orders[4], orders[5], inverses[4], inverses[5])
    mix = Mamba2(d_model=64, d_state=16, d_conv=4, expand=2, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                 origina_list_reversal=lists[3]).to(gpu)
    with torch.no_grad():
        mix.norm.weight.add_(torch.randn_like(mix.norm.weight) * 0.1)
        mix.D.add_(torch.randn_like(mix.D) * 0.1)
    x = torch.randn(3, n * n, 64, device=gpu, requires_grad=True)
    dy = torch.randn(3, n * n, 64, device=gpu)
    y = mix(x, "spiral")
    (y * dy).sum().backward()
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mix.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    yr = mamba2_spiral_forward_ref(x64, params, lists, headdim=64, dtype=torch.float64)
    (yr * dy.cpu().double()).sum().backward()
    assert rel_l2(y.detach().cpu(), yr.detach()) <= 1e-4
    assert rel_l2(x.grad.cpu(), x64.grad) <= 5e-4
    for k, p in mix.named_parameters():
        assert rel_l2(p.grad.cpu(), params[k].grad) <= 5e-4, k


def test_mamba2_mixer_inference_chunk_parallel_scan(gpu):
    """Under no_grad at L = 196 the small launch takes the chunk-parallel scan in its one-decay-per-head form
    (scan_fwd_chunked.h with DM_FLAG_A_SHARED); same oracle as above."""
    from diffma_amd.mamba2 import Mamba2
    from diffma_amd.tools import spiral
    from oracle.mamba2_ref import mamba2_spiral_forward_ref

    torch.manual_seed(2)
    n = 14
    orders, inverses = spiral(n)
    lists = (orders[2], orders[3], inverses[2], inverses[3])
    mix = Mamba2(d_model=64, d_state=16, d_conv=4, expand=2, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                 origina_list_reversal=lists[3]).to(gpu).eval()
    x = torch.randn(2, n * n, 64, device=gpu)
    with torch.no_grad():
        y = mix(x, "spiral")
        params = {k: v.detach().cpu().double() for k, v in mix.state_dict().items()}
        yr = mamba2_spiral_forward_ref(x.cpu().double(), params, lists, headdim=64, dtype=torch.float64)
    assert rel_l2(y.cpu(), yr) <= 1e-4, rel_l2(y.cpu(), yr)


def test_mamba_split_conv1d_scan_combined_signature(gpu):
    """The reference's keyword call (block/mamba2.py:392-410) against the oracle restatement, incl. a strided input."""
    from diffma_amd.selective_scan_interface import mamba_split_conv1d_scan_combined
    from oracle.mamba2_ref import mamba_split_conv1d_scan_combined_ref

    gen = torch.Generator().manual_seed(8)
    B, L, H, P, N, dm = 2, 49, 2, 64, 16, 48
    dim = H * P
    mk = lambda *s, sc=1.0: torch.randn(*s, generator=gen) * sc
    zx = mk(B, 3, L, 2 * dim + 2 * N + H)[:, 1]                     # strided slice like CrossScan's xs[:, k]
    cw, cb = mk(dim + 2 * N, 4, sc=0.4), mk(dim + 2 * N, sc=0.1)
    dt_bias, A, D = mk(H, sc=0.5), -(torch.rand(H, generator=gen) * 4 + 0.5), mk(H)
    nw, ow = 1 + mk(dim, sc=0.1), mk(dm, dim, sc=0.1)
    kw = dict(chunk_size=256, seq_idx=None, activation="silu", rmsnorm_weight=None, rmsnorm_eps=1e-5, outproj_weight=None,
              outproj_bias=None, headdim=P, ngroups=1, norm_before_gate=False)
    to = lambda t: t.to(gpu)
    got = mamba_split_conv1d_scan_combined(to(zx), to(cw), to(cb), to(dt_bias), to(A), D=to(D),
                                           **{**kw, "rmsnorm_weight": to(nw), "outproj_weight": to(ow)})
    ref = mamba_split_conv1d_scan_combined_ref(zx.double(), cw, cb, dt_bias, A, D=D, **{**kw, "rmsnorm_weight": nw, "outproj_weight": ow})
    assert got.shape == (B, L, dm) and rel_l2(got.cpu(), ref) <= 1e-4


# ---- fused block elementwise kernels (csrc/block_ops.hip) vs the eager ATen formulation ------------------------------------
@pytest.mark.parametrize("amp", [None, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("hidden,n", [(64, 4), (512, 14)])
def test_block_fused_elementwise_matches_eager(gpu, amp, hidden, n):
    from diffma_amd.mamba_block import Spiral_MambaBlock
    from diffma_amd.tools import spiral

    torch.manual_seed(0)
    orders, inverses = spiral(n)
    blk = Spiral_MambaBlock(D_dim=hidden, E_dim=2 * hidden, dt_rank=16, dim_inner=2 * hidden, d_state=16, token_list=orders[0],
                            token_list_reversal=orders[1], origina_list=inverses[0], origina_list_reversal=inverses[1]).to(gpu)
    with torch.no_grad():
        for p in blk.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn_like(p) * 0.05)
        blk.norm1.weight.add_(torch.randn_like(blk.norm1.weight) * 0.1)
        blk.norm1.bias.add_(torch.randn_like(blk.norm1.bias) * 0.1)
    B = 3
    x0 = torch.randn(B, n * n, hidden, device=gpu)
    c0 = torch.randn(B, 2 * hidden, device=gpu)
    w = torch.sigmoid(torch.randn(B, n * n, 1, device=gpu))
    dy = torch.randn(B, n * n, hidden, device=gpu)

    def run(fused):
        blk.fused_elementwise = fused
        blk.zero_grad(set_to_none=True)
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            y = blk(x, c, w)
        (y.float() * dy).sum().backward()
        return y.detach().float(), x.grad, c.grad, {k: p.grad.clone() for k, p in blk.named_parameters()}

    ya, xa, ca, ga = run(True)
    yb, xb, cb, gb = run(False)
    tol = 2e-2 if amp else 2e-5
    assert rel_l2(ya, yb) <= tol
    assert rel_l2(xa, xb) <= 2 * tol and rel_l2(ca, cb) <= 2 * tol
    for k in ga:
        # a 1-element bf16 gradient (the fusion head's bias) is a sum with cancellation: both paths are equally far from fp32
        lim = 3 * tol if (amp is None or ga[k].numel() >= 64) else 0.25
        assert rel_l2(ga[k], gb[k]) <= lim, k
    blk.fused_elementwise = True


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_block_wider_than_k8_takes_eager_form(gpu, amp):
    """D_dim = 640: LN(cat[x_ssm, w_ssm]) normalises rows of 1280 values, more than K8 (csrc/block_ops.hip) takes.  The block
    must run forward and backward (hip_ops.ln_mod_supported sends it to the eager formulation) and match fused_elementwise=False
    within the bounds of test_block_fused_elementwise_matches_eager."""
    from diffma_amd import hip_ops
    from diffma_amd.mamba_block import Spiral_MambaBlock
    from diffma_amd.tools import spiral

    hidden, n, B = 640, 4, 2
    assert hip_ops.ln_mod_supported(hidden) and not hip_ops.ln_mod_supported(2 * hidden)
    torch.manual_seed(0)
    orders, inverses = spiral(n)
    blk = Spiral_MambaBlock(D_dim=hidden, E_dim=2 * hidden, dt_rank=16, dim_inner=2 * hidden, d_state=16, token_list=orders[0],
                            token_list_reversal=orders[1], origina_list=inverses[0], origina_list_reversal=inverses[1]).to(gpu)
    with torch.no_grad():
        for p in blk.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn_like(p) * 0.05)
    x0 = torch.randn(B, n * n, hidden, device=gpu)
    c0 = torch.randn(B, 2 * hidden, device=gpu)
    w = torch.sigmoid(torch.randn(B, n * n, 1, device=gpu))
    dy = torch.randn(B, n * n, hidden, device=gpu)

    def run(fused):
        blk.fused_elementwise = fused
        blk.zero_grad(set_to_none=True)
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            y = blk(x, c, w)
        (y.float() * dy).sum().backward()
        torch.cuda.synchronize()
        return y.detach().float(), x.grad, c.grad, {k: p.grad.clone() for k, p in blk.named_parameters()}

    try:
        ya, xa, ca, ga = run(True)
    finally:
        blk.fused_elementwise = True
    yb, xb, cb, gb = run(False)
    tol = 2e-2 if amp else 2e-5
    assert torch.isfinite(ya).all() and rel_l2(ya, yb) <= tol
    assert rel_l2(xa, xb) <= 2 * tol and rel_l2(ca, cb) <= 2 * tol
    for k in ga:
        lim = 3 * tol if (amp is None or ga[k].numel() >= 64) else 0.25
        assert rel_l2(ga[k], gb[k]) <= lim, k
    blk.fused_elementwise = True


def test_graphed_denoiser_matches_eager(gpu):
    """hipGraph replay of the denoiser == eager call, and a full respaced p_sample_loop through it is reproducible."""
    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.graphed import GraphedDenoiser

    g, sd, net, inp = _g5(gpu)
    gd = GraphedDenoiser(net, inp["x"], inp["t"], inp["y"], inp["y2"], inp["w"])
    with torch.no_grad():
        eager = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"])
        x2 = torch.randn_like(inp["x"])
        t2 = torch.tensor([500, 1], device=gpu)
        e2 = net(x2, t2, y=inp["y"], y2=inp["y2"], w=inp["w"])
    torch.testing.assert_close(gd(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).clone(), eager, rtol=0, atol=0)
    torch.testing.assert_close(gd(x2, t2, y=inp["y"], y2=inp["y2"], w=inp["w"]).clone(), e2, rtol=0, atol=0)
    d = create_diffusion("10")
    kw = dict(y=inp["y"], y2=inp["y2"], w=inp["w"])
    z = torch.randn(2, 4, 8, 8, device=gpu)
    torch.manual_seed(3)
    a = d.p_sample_loop(gd, z.shape, z, clip_denoised=False, model_kwargs=kw, device=gpu)
    torch.manual_seed(3)
    b = d.p_sample_loop(net.forward, z.shape, z, clip_denoised=False, model_kwargs=kw, device=gpu)
    torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_graphed_train_step(gpu):
    """The whole optimisation step replayed from a hipGraph: the loss is finite and falls on a fixed batch, the weights move,
    the EMA follows its recurrence exactly, and two identically seeded instances produce the same loss sequence."""
    import copy

    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.graphed import GraphedTrainStep

    g, sd, net0, inp = _g5(gpu)
    d = create_diffusion("")
    B = inp["x"].shape[0]

    def run(steps):
        torch.manual_seed(11)
        net = copy.deepcopy(net0).train()
        ema = copy.deepcopy(net).requires_grad_(False)
        opt = torch.optim.AdamW(net.parameters(), lr=2e-3, weight_decay=0, fused=True, capturable=True)
        gs = GraphedTrainStep(net, ema, opt, d, inp["x"], torch.zeros(B, device=gpu, dtype=torch.long), inp["y"], inp["y2"], inp["w"],
                              ema_decay=0.9, warmup=2)
        tg = torch.Generator(device=gpu).manual_seed(5)
        losses = []
        for _ in range(steps):
            t = torch.randint(0, d.num_timesteps, (B,), device=gpu, generator=tg)
            ema_before = [p.detach().clone() for p in ema.parameters()]
            losses.append(float(gs.step(inp["x"], t, inp["y"], inp["y2"], inp["w"])))
        return net, ema, ema_before, losses

    net, ema, ema_before, losses = run(12)
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert sum(losses[-4:]) < sum(losses[:4]), losses                    # the same batch every step: the loss must come down
    moved = sum(float((a.detach() - b.detach()).abs().sum()) for a, b in zip(net.parameters(), net0.parameters()))
    assert moved > 0
    for e_new, e_old, p in zip(ema.parameters(), ema_before, net.parameters()):
        torch.testing.assert_close(e_new, 0.9 * e_old + 0.1 * p.detach(), rtol=1e-5, atol=1e-6)
    _, _, _, losses2 = run(12)
    assert losses == losses2


def test_graphed_train_step_drops_a_non_finite_step_on_the_device(gpu):
    """A replayed graph cannot branch on the host: a batch that yields non-finite gradients must leave weights, AdamW moments and
    the step counter untouched (found_inf computed inside the graph), be counted in `skipped`, and the run must go
    on with the next batch -- the graphed counterpart of the reference's `continue` (train.py:254-256)."""
    import copy

    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.graphed import GraphedTrainStep

    g, sd, net0, inp = _g5(gpu)
    d = create_diffusion("")
    B = inp["x"].shape[0]
    torch.manual_seed(3)
    net = copy.deepcopy(net0).train()
    ema = copy.deepcopy(net).requires_grad_(False)
    opt = torch.optim.AdamW(net.parameters(), lr=2e-3, weight_decay=0, fused=True, capturable=True)
    t = torch.full((B,), 300, device=gpu, dtype=torch.long)
    gs = GraphedTrainStep(net, ema, opt, d, inp["x"], t, inp["y"], inp["y2"], inp["w"], ema_decay=0.9, warmup=2)
    gs.step(inp["x"], t, inp["y"], inp["y2"], inp["w"])
    before = [p.detach().clone() for p in net.parameters()]
    ema_before = [p.detach().clone() for p in ema.parameters()]
    steps_before = [float(st["step"]) for st in opt.state.values()]
    bad = inp["x"].clone()
    bad[0, 0, 0, 0] = float("nan")
    loss = gs.step(bad, t, inp["y"], inp["y2"], inp["w"])
    assert not torch.isfinite(loss).all() and float(gs.skipped) == 1.0
    assert all(torch.equal(a.detach(), b) for a, b in zip(net.parameters(), before))
    assert [float(st["step"]) for st in opt.state.values()] == steps_before
    for e_new, e_old, p in zip(ema.parameters(), ema_before, net.parameters()):   # one ordinary EMA step towards the UNCHANGED weights: finite, bounded
        torch.testing.assert_close(e_new, 0.9 * e_old + 0.1 * p.detach(), rtol=1e-5, atol=1e-6)
    loss = gs.step(inp["x"], t, inp["y"], inp["y2"], inp["w"])               # the run continues
    assert torch.isfinite(loss).all() and float(gs.skipped) == 1.0
    assert any(not torch.equal(a.detach(), b) for a, b in zip(net.parameters(), before))


# ---- baseline scan orders on the same kernels (tests/golden/g9_baseline_blocks.npz) ------------------------
def _g9(gpu, tag):
    from diffma_amd.model import DiffMa

    g = np.load(os.path.join(G, "g9_baseline_blocks.npz"))
    pre = tag + ".sd."
    sd = {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}
    depth = int(g[f"{tag}.depth"])
    net = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=depth, d_state=16, block_type=tag.split(".")[-1],
                 use_mamba2=tag.startswith("m2."))
    net.load_state_dict(sd)
    net = net.to(gpu).eval()
    inp = {k: torch.from_numpy(g[f"{tag}.{k}"]).to(gpu) for k in ("x", "t", "y", "y2", "w")}
    return g, sd, net, inp, depth


@pytest.mark.parametrize("bt", ["zig", "vim", "vmamba", "efficientVMamba", "m2.zig", "m2.vim", "m2.vmamba"])
def test_baseline_blocks_forward_match_reference(gpu, bt):
    """ZigMa / ViM / VMamba / EfficientVMamba denoisers on the HIP operator against the output of the reference's own
    classes (operator = fp64 oracle stub): fp32 rel-L2 <= 1e-3 per block and at the output, bf16 autocast <= 2e-2."""
    g, sd, net, inp, depth = _g9(gpu, bt)
    acts = {}
    hooks = [b.register_forward_hook(lambda m, i, o, k=k: acts.__setitem__(k, o.detach().cpu())) for k, b in enumerate(net.blocks)]
    with torch.no_grad():
        out = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).cpu()
    for h in hooks:
        h.remove()
    ref = torch.from_numpy(g[f"{bt}.out"])
    for k in range(depth):
        assert rel_l2(acts[k], torch.from_numpy(g[f"{bt}.act.block{k}"])) <= 1e-3, (bt, k)
    assert rel_l2(out, ref) <= 1e-3, rel_l2(out, ref)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).float().cpu()
    assert rel_l2(out16, ref) <= 2e-2


@pytest.mark.parametrize("scan_type", ["zigma", "vim", "vim-token", "vmamba", "eff"])
def test_baseline_mixer_forward_backward_match_oracle_autograd(gpu, scan_type):
    """Mamba.forward(x, scan_type) and its gradients (inputs and all parameters) against fp64 autograd through the oracle."""
    from diffma_amd.mamba import Mamba
    from diffma_amd.tools import vmamba_, zig
    from oracle.mamba_ref import mamba_baseline_forward_ref

    torch.manual_seed(11)
    n, dm, Bsz = 6, 64, 3
    L = n * n
    st = scan_type.split("-")[0]
    lists = zig(n, 3) if st == "zigma" else (vmamba_(n) if st == "vmamba" else None)
    kw = dict(token_list=lists[0], origina_list=lists[1]) if lists else {}
    mix = Mamba(d_model=dm, d_state=16, d_conv=4, expand=2, **kw)
    with torch.no_grad():
        mix.A_log.add_(torch.randn_like(mix.A_log) * 0.1)
        mix.D.add_(torch.randn_like(mix.D) * 0.1)
    if scan_type == "vim-token":
        mix.vim_flip = "token"
    mix = mix.to(gpu)
    x = torch.randn(Bsz, L, dm)
    gout = torch.randn(Bsz, L, dm)
    xg = x.to(gpu).requires_grad_(True)
    out = mix(xg, st)
    out.backward(gout.to(gpu))

    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mix.named_parameters()}
    xr = x.double().requires_grad_(True)
    if scan_type == "vim-token":                 # the intended ViM: flip the second output back along the token axis
        from oracle.mamba_ref import mamba_inner_ref
        xz = torch.einsum("ed,bld->bel", params["in_proj.weight"], xr)
        A = -torch.exp(params["A_log"])
        inner = lambda t: mamba_inner_ref(t, params["conv1d.weight"], params["conv1d.bias"], params["x_proj.weight"],
                                          params["dt_proj.weight"], params["out_proj.weight"], None, A, None, None, params["D"],
                                          delta_bias=params["dt_proj.bias"], delta_softplus=True, dtype=torch.float64)
        ref = (inner(xz) + torch.flip(inner(torch.flip(xz, [2])), [1])) / 2
    else:
        ref = mamba_baseline_forward_ref(xr, params, st, lists, dtype=torch.float64)
    ref.backward(gout.double())
    assert rel_l2(out.detach().cpu(), ref.detach()) <= 1e-4
    assert rel_l2(xg.grad.cpu(), xr.grad) <= 1e-3
    for k, v in mix.named_parameters():
        assert rel_l2(v.grad.cpu(), params[k].grad) <= 2e-3, k


@pytest.mark.parametrize("scan_type", ["zigma", "vim", "vmamba"])
def test_baseline_mamba2_mixer_forward_backward_match_oracle_autograd(gpu, scan_type):
    """Mamba2.forward(x, scan_type) and its gradients against fp64 autograd through the oracle."""
    from diffma_amd.mamba2 import Mamba2
    from diffma_amd.tools import vmamba_, zig
    from oracle.mamba2_ref import mamba2_baseline_forward_ref

    torch.manual_seed(12)
    n, dm, Bsz = 6, 64, 3
    L = n * n
    lists = zig(n, 6) if scan_type == "zigma" else (vmamba_(n) if scan_type == "vmamba" else None)
    kw = dict(token_list=lists[0], origina_list=lists[1]) if lists else {}
    mix = Mamba2(d_model=dm, d_state=16, d_conv=4, expand=2, **kw)
    with torch.no_grad():
        mix.norm.weight.add_(torch.randn_like(mix.norm.weight) * 0.1)
        mix.D.add_(torch.randn_like(mix.D) * 0.1)
    mix = mix.to(gpu)
    x, gout = torch.randn(Bsz, L, dm), torch.randn(Bsz, L, dm)
    xg = x.to(gpu).requires_grad_(True)
    out = mix(xg, scan_type)
    out.backward(gout.to(gpu))
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mix.named_parameters()}
    xr = x.double().requires_grad_(True)
    ref = mamba2_baseline_forward_ref(xr, params, scan_type, lists, headdim=mix.headdim, dtype=torch.float64)
    ref.backward(gout.double())
    assert rel_l2(out.detach().cpu(), ref.detach()) <= 1e-4
    assert rel_l2(xg.grad.cpu(), xr.grad) <= 1e-3
    for k, v in mix.named_parameters():
        assert rel_l2(v.grad.cpu(), params[k].grad) <= 2e-3, k


def test_fp16_autocast_with_gradscaler_reference_mode(gpu):
    """The reference's own mixed-precision mode (train.py:95,247-263: fp16 autocast + GradScaler) on the HIP path: forward
    within the fp16 end-to-end tolerance of the fp32 golden output, and two scaled optimisation steps that stay finite."""
    from diffma_amd.diffusion import create_diffusion

    g, sd, net, inp = _g5(gpu)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).float().cpu()
    assert rel_l2(out, torch.from_numpy(g["out"])) <= 5e-3
    net.train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=0)
    scaler = torch.amp.GradScaler("cuda")
    d = create_diffusion("")
    z, tt = torch.from_numpy(g["loss_z"]).to(gpu), torch.from_numpy(g["loss_t"]).to(gpu)
    before = net.blocks[0].mamba1.in_proj.weight.detach().clone()
    for _ in range(2):
        with torch.autocast("cuda", dtype=torch.float16):
            loss = d.training_losses(net, z, tt, dict(y=inp["y"], y2=inp["y2"], w=inp["w"]))["loss"].mean()
        assert torch.isfinite(loss)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        opt.zero_grad(set_to_none=True)
    assert scaler.get_scale() > 0
    assert not torch.equal(before, net.blocks[0].mamba1.in_proj.weight.detach())


def test_two_stream_mixers_match_single_stream(gpu):
    """The opt-in two-stream mode of the block (mamba_block.Spiral_MambaBlock.overlap_mixers): same loss and gradients as
    the single-stream default (the kernels and their order per mixer are identical, only the queues differ)."""
    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.mamba_block import Spiral_MambaBlock

    g, sd, net, inp = _g5(gpu)
    net.train()
    d = create_diffusion("")
    z, nz, tt = (torch.from_numpy(g[k]).to(gpu) for k in ("loss_z", "loss_noise", "loss_t"))

    def run():
        net.zero_grad(set_to_none=True)
        loss = d.training_losses(net, z, tt, dict(y=inp["y"], y2=inp["y2"], w=inp["w"]), noise=nz)["loss"].mean()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    l0, g0 = run()
    prev = Spiral_MambaBlock.overlap_mixers
    Spiral_MambaBlock.overlap_mixers = True
    try:
        l1, g1 = run()
    finally:
        Spiral_MambaBlock.overlap_mixers = prev
    assert torch.equal(l0, l1)
    assert g0.keys() == g1.keys()
    for k in g0:
        torch.testing.assert_close(g1[k], g0[k], rtol=1e-5, atol=1e-7, msg=k)


# ---- G10: the HIP operators against the arithmetic the REFERENCE ITSELF holds (Mamba.step / Mamba2.step, token by token) ----
# tests/golden/g10_reference_step.npz is produced by tools/gen_golden.py from block/mamba.py:405-448 and block/mamba2.py:715-775
# alone -- no oracle function takes part, so these tests pin the HIP path directly to reference-held code.
def _g10(tag):
    g = np.load(os.path.join(G, "g10_reference_step.npz"))
    sd = {k[len(tag) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + ".sd.")}
    extra = {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + ".") and ".sd." not in k}
    return sd, extra


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2), (torch.float16, 4e-3)])
@pytest.mark.parametrize("tag", ["m1.a", "m1.b", "m1.c"])
def test_mamba_inner_fn_matches_reference_step(gpu, tag, dtype, tol):
    """mamba_inner_fn (reference call: block/mamba.py:346) on the (B, 2D, L) in_proj output vs the stacked outputs of the
    reference's own Mamba.step(); fp32 rel-L2 <= 1e-4, bf16 <= 2e-2, fp16 <= 4e-3."""
    from diffma_amd.selective_scan_interface import mamba_inner_fn, selective_scan_fn

    sd, e = _g10(tag)
    hidden, want = torch.from_numpy(e["hidden"]), torch.from_numpy(e["out"])
    f = lambda t: t.float().to(gpu)
    xz = torch.einsum("ed,bld->bel", sd["in_proj.weight"], hidden)                  # (B, 2Din, L) fp64, block/mamba.py:333-337
    A = f(torch.from_numpy(e["A"]))
    out = mamba_inner_fn(xz.to(dtype).to(gpu), f(sd["conv1d.weight"]), f(sd["conv1d.bias"]), f(sd["x_proj.weight"]).to(dtype),
                         f(sd["dt_proj.weight"]).to(dtype), f(sd["out_proj.weight"]).to(dtype), None, A, None, None, f(sd["D"]),
                         delta_bias=f(sd["dt_proj.bias"]), delta_softplus=True)
    assert out.shape == want.shape
    assert rel_l2(out.float().cpu(), want) <= tol, rel_l2(out.float().cpu(), want)
    if dtype == torch.float32:                       # selective_scan_fn + return_last_state against the reference's final ssm_state
        from oracle.mamba_ref import causal_conv1d_ref
        Din, R, N = sd["D"].shape[0], sd["dt_proj.weight"].shape[1], A.shape[1]
        xc = causal_conv1d_ref(xz[:, :Din], sd["conv1d.weight"].reshape(Din, -1), sd["conv1d.bias"], activation="silu")
        x_dbl = torch.einsum("bdl,ed->ble", xc, sd["x_proj.weight"])
        delta = torch.einsum("blr,dr->bdl", x_dbl[..., :R], sd["dt_proj.weight"])
        y, last = selective_scan_fn(f(xc), f(delta), A, f(x_dbl[..., R:R + N].permute(0, 2, 1)), f(x_dbl[..., R + N:].permute(0, 2, 1)),
                                    f(sd["D"]), z=f(xz[:, Din:]), delta_bias=f(sd["dt_proj.bias"]), delta_softplus=True,
                                    return_last_state=True)
        assert rel_l2(last.cpu(), torch.from_numpy(e["last_state"])) <= 1e-4
        assert rel_l2(torch.einsum("bdl,ed->ble", y.cpu().double(), sd["out_proj.weight"]), want) <= 1e-4


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize("tag", ["m2.a", "m2.b", "m2.c", "m2.d"])
def test_mamba_split_conv1d_scan_combined_matches_reference_step(gpu, tag, dtype, tol):
    """mamba_split_conv1d_scan_combined (reference call: block/mamba2.py:392-410) vs the reference's own Mamba2.step();
    m2.a / m2.b run without the gated RMSNorm (held by the reference end to end), m2.c / m2.d with it."""
    from diffma_amd.selective_scan_interface import mamba_split_conv1d_scan_combined

    sd, e = _g10(tag)
    hidden, want = torch.from_numpy(e["hidden"]), torch.from_numpy(e["out"])
    rms = bool(int(e["rmsnorm"]))
    f = lambda t: t.float().to(gpu)
    zx = (hidden @ sd["in_proj.weight"].t()).to(dtype).to(gpu)
    out = mamba_split_conv1d_scan_combined(
        zx, f(sd["conv1d.weight"]).squeeze(1), f(sd["conv1d.bias"]), f(sd["dt_bias"]), f(torch.from_numpy(e["A"])), D=f(sd["D"]),
        chunk_size=256, seq_idx=None, activation="silu", rmsnorm_weight=f(sd["norm.weight"]) if rms else None, rmsnorm_eps=1e-5,
        outproj_weight=f(sd["out_proj.weight"]).to(dtype), outproj_bias=None, headdim=int(e["headdim"]), ngroups=1, norm_before_gate=False)
    assert out.shape == want.shape
    assert rel_l2(out.float().cpu(), want) <= tol, rel_l2(out.float().cpu(), want)


@pytest.mark.parametrize("tag", ["m1.b", "m1.c"])
def test_mamba_module_matches_reference_step(gpu, tag):
    """The product Mamba module loaded with the reference module's state dict: forward over the whole sequence with identity
    scan tables ('zigma' with the identity permutation = one causal direction) equals the reference's step-by-step decode."""
    from diffma_amd.mamba import Mamba

    sd, e = _g10(tag)
    hidden, want = torch.from_numpy(e["hidden"]), torch.from_numpy(e["out"])
    L, dm = hidden.shape[1], hidden.shape[2]
    ident = list(range(L))
    mix = Mamba(d_model=dm, d_state=16, d_conv=4, expand=2, token_list=ident, origina_list=ident)
    mix.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    mix = mix.to(gpu)
    with torch.no_grad():
        out = mix(hidden.float().to(gpu), "zigma")
    assert rel_l2(out.cpu(), want) <= 1e-4, rel_l2(out.cpu(), want)


def test_fused_conv_xproj_path_in_the_mixer(gpu, monkeypatch):
    """The fused conv + x_proj kernel (K3x) is selected by launch size; force it on at test sizes and repeat the bf16 mixer
    forward/backward check against fp64 oracle autograd, the bf16 G5 denoiser, and the bf16/fp16 G10 reference-step parity."""
    from diffma_amd import hip_ops
    from diffma_amd.selective_scan_interface import mamba_inner_fn

    calls = {"n": 0}
    real = hip_ops.gather_conv1d_xproj_fwd

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    real_b = hip_ops.gather_conv1d_xproj_bwd

    def counted_b(*a, **k):
        calls["b"] = calls.get("b", 0) + 1
        return real_b(*a, **k)

    monkeypatch.setattr(hip_ops, "XPROJ_FUSED_MIN_SEQS", 1)
    monkeypatch.setattr(hip_ops, "XPROJ_FUSED_BWD", True)
    monkeypatch.setattr(hip_ops, "gather_conv1d_xproj_fwd", counted)
    monkeypatch.setattr(hip_ops, "gather_conv1d_xproj_bwd", counted_b)
    _mixer_case(gpu, torch.bfloat16, 2e-2)          # d_model 64: dim 128, 36 projection rows -> fused forward, unfused backward
    assert calls["n"] >= 1
    _mixer_case(gpu, torch.bfloat16, 2e-2, d_model=512)   # dim 1024, 32 + 32 = 64 projection rows (every DiffMa-*) -> both fused kernels
    assert calls.get("b", 0) >= 1
    g, sd, net, inp = _g5(gpu)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=inp["w"]).float().cpu()
    assert rel_l2(out, torch.from_numpy(g["out"])) <= 2e-2
    n0 = calls["n"]
    for tag in ("m1.b", "m1.c"):
        for dtype, tol in ((torch.bfloat16, 2e-2), (torch.float16, 4e-3)):
            sd10, e = _g10(tag)
            hidden, want = torch.from_numpy(e["hidden"]), torch.from_numpy(e["out"])
            f = lambda t: t.float().to(gpu)
            xz = torch.einsum("ed,bld->bel", sd10["in_proj.weight"], hidden)
            o = mamba_inner_fn(xz.to(dtype).to(gpu), f(sd10["conv1d.weight"]), f(sd10["conv1d.bias"]), f(sd10["x_proj.weight"]).to(dtype),
                               f(sd10["dt_proj.weight"]).to(dtype), f(sd10["out_proj.weight"]).to(dtype), None, f(torch.from_numpy(e["A"])),
                               None, None, f(sd10["D"]), delta_bias=f(sd10["dt_proj.bias"]), delta_softplus=True)
            assert rel_l2(o.float().cpu(), want) <= tol, (tag, dtype, rel_l2(o.float().cpu(), want))
    assert calls["n"] > n0


@pytest.mark.parametrize("d_model,expect_calls", [(256, 1), (64, 0)])
def test_mamba2_mixer_inference_on_the_mfma_ssd_prototype(gpu, monkeypatch, d_model, expect_calls):
    """The matrix-pipe SSD forward (csrc/ssd.hip; DIFFMA_SSD_MFMA, on by default) inside the Mamba-2 mixer under no_grad + bf16
    autocast, against the fp64 oracle mixer.  The kernel moves 16-byte row pieces: with nheads % 8 != 0 (d_model 64: 2 heads) the
    z rows of the in_proj output are not 16-byte aligned and the mixer must take the A-shared scan instead -- same result."""
    from diffma_amd import hip_ops
    from diffma_amd.mamba2 import Mamba2
    from diffma_amd.tools import spiral
    from oracle.mamba2_ref import mamba2_spiral_forward_ref

    calls = {"n": 0}
    real = hip_ops.ssd_fwd

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(hip_ops, "SSD_MFMA", True)
    monkeypatch.setattr(hip_ops, "ssd_fwd", counted)
    torch.manual_seed(4)
    n = 14
    orders, inverses = spiral(n)
    lists = (orders[6], orders[7], inverses[6], inverses[7])
    mix = Mamba2(d_model=d_model, d_state=16, d_conv=4, expand=2, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                 origina_list_reversal=lists[3]).to(gpu).eval()
    x = torch.randn(2, n * n, d_model, device=gpu)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = mix(x, "spiral").float()
    assert calls["n"] == expect_calls
    params = {k: v.detach().cpu().double() for k, v in mix.state_dict().items()}
    yr = mamba2_spiral_forward_ref(x.cpu().double(), params, lists, headdim=64, dtype=torch.float64)
    assert rel_l2(y.cpu(), yr) <= 2e-2, rel_l2(y.cpu(), yr)


@pytest.mark.parametrize("n", [14, 7])
def test_mamba2_mixer_training_on_the_matrix_pipe(gpu, monkeypatch, n):
    """Mamba-2 mixer forward + backward under bf16 autocast with 8 heads (16-byte aligned rows): the autograd node must run
    csrc/ssd.hip forward and csrc/ssd_bwd.hip backward (no scan launch at all), and every gradient must match fp64 autograd
    through the oracle mixer within bf16 tolerance; the same step on the A-shared scan pair (DIFFMA_SSD_MFMA_BWD off) agrees too."""
    from diffma_amd import hip_ops
    from diffma_amd.mamba2 import Mamba2
    from diffma_amd.tools import spiral
    from oracle.mamba2_ref import mamba2_spiral_forward_ref

    calls = {"ssd_fwd": 0, "ssd_bwd": 0, "scan_fwd": 0, "scan_bwd": 0}
    for name in calls:
        real = getattr(hip_ops, name)
        monkeypatch.setattr(hip_ops, name, (lambda real, name: lambda *a, **k: (calls.__setitem__(name, calls[name] + 1), real(*a, **k))[1])(real, name))
    torch.manual_seed(n)
    orders, inverses = spiral(n)
    lists = (orders[2], orders[3], inverses[2], inverses[3])
    d_model = 256
    mix = Mamba2(d_model=d_model, d_state=16, d_conv=4, expand=2, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                 origina_list_reversal=lists[3]).to(gpu)
    with torch.no_grad():
        mix.norm.weight.add_(torch.randn_like(mix.norm.weight) * 0.1)
        mix.D.add_(torch.randn_like(mix.D) * 0.1)
    x = torch.randn(2, n * n, d_model, device=gpu, requires_grad=True)
    dy = torch.randn(2, n * n, d_model, device=gpu)

    def step():
        x.grad = None
        mix.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mix(x, "spiral")
        (y.float() * dy).sum().backward()
        return y.detach().float().cpu(), x.grad.detach().cpu().clone(), {k: p.grad.detach().float().cpu().clone() for k, p in mix.named_parameters()}

    y, gx, gp = step()
    assert calls == {"ssd_fwd": 1, "ssd_bwd": 1, "scan_fwd": 0, "scan_bwd": 0}, calls
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mix.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    yr = mamba2_spiral_forward_ref(x64, params, lists, headdim=64, dtype=torch.float64)
    (yr * dy.cpu().double()).sum().backward()
    assert rel_l2(y, yr.detach()) <= 2e-2, rel_l2(y, yr.detach())
    assert rel_l2(gx, x64.grad) <= 3e-2, rel_l2(gx, x64.grad)
    for k in gp:
        assert rel_l2(gp[k], params[k].grad) <= 4e-2, (k, rel_l2(gp[k], params[k].grad))
    monkeypatch.setattr(hip_ops, "SSD_MFMA_BWD", False)                     # training back on the scan pair
    y2, gx2, gp2 = step()
    assert calls["scan_fwd"] == 1 and calls["scan_bwd"] == 1 and calls["ssd_bwd"] == 1
    assert rel_l2(y, y2) <= 2e-2 and rel_l2(gx, gx2) <= 3e-2
    for k in gp:
        assert rel_l2(gp[k], gp2[k]) <= 4e-2, (k, rel_l2(gp[k], gp2[k]))


# ------------------------------------------------------------------------------------------------------------------
# BASELINE.json's configurations at their REAL depth and width: the factory model, batch 1, one forward on
# the device against the CPU oracle (functional restatement on the same state dict; fp32, rel-L2 <= 1e-3).
# ------------------------------------------------------------------------------------------------------------------
def _rerandomize(net, seed):
    """The reference init zeroes the output layers / adaLN / dt_proj.bias (SURVEY.md A.4-1,3): the stock output is exactly 0."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.requires_grad and float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
            if name.endswith("dt_proj.bias"):
                dt = torch.exp(torch.rand(p.shape, generator=gen) * (np.log(0.1) - np.log(0.001)) + np.log(0.001))
                p.copy_(dt + torch.log(-torch.expm1(-dt)))


@pytest.mark.parametrize("name,kw", [("DiffMa-B/4", {}), ("DiffMa-L/2", {}), ("DiffMa-XL/2", dict(use_mamba2=True)), ("DiffMa-XXL/2", {})])
def test_baseline_config_models_match_oracle_at_full_size(gpu, name, kw):
    from diffma_amd.model import DiffMa_models
    from oracle.model_ref import diffma_forward_ref

    torch.manual_seed(11)
    net = DiffMa_models[name](input_size=28, dt_rank=16, d_state=16, **kw).eval()
    _rerandomize(net, 12)
    patch, depth = int(name.split("/")[1]), len(net.blocks)
    L = (28 // patch) ** 2
    g = torch.Generator().manual_seed(13)
    x, y, y2 = torch.randn(1, 4, 28, 28, generator=g), torch.randn(1, 512, generator=g), torch.randn(1, L, 512, generator=g)
    w = torch.sigmoid(torch.randn(1, L, 1, generator=g))
    t = torch.tensor([437])
    # the oracle's torch code runs on the device for the full-size models (ATen fp32 kernels; 106 s of host time for XXL/2 otherwise)
    odev = torch.device("cpu") if os.environ.get("DIFFMA_TEST_ORACLE_ON_HOST") == "1" else gpu
    sd = {k: v.detach().clone().to(odev) for k, v in net.state_dict().items()}
    ref, blocks = diffma_forward_ref(sd, x.to(odev), t.to(odev), y.to(odev), y2.to(odev), w.to(odev), patch_size=patch, depth=depth,
                                     dtype=torch.float32, return_blocks=True, use_mamba2=kw.get("use_mamba2", False))
    ref, blocks = ref.cpu(), [b.cpu() for b in blocks]
    del sd
    net = net.to(gpu)
    acts = {}
    hooks = [b.register_forward_hook(lambda m, i, o, k=k: acts.__setitem__(k, o.detach().cpu())) for k, b in enumerate(net.blocks)]
    with torch.no_grad():
        out = net(x.to(gpu), t.to(gpu), y=y.to(gpu), y2=y2.to(gpu), w=w.to(gpu)).cpu()
    for h in hooks:
        h.remove()
    assert float(ref.abs().mean()) > 1e-3                          # a live output, not the zero-init one
    assert rel_l2(out, ref) <= 1e-3, rel_l2(out, ref)
    for k in (0, depth // 2, depth - 1):                           # first, the block where the long skips start, last
        assert rel_l2(acts[k], blocks[k]) <= 1e-3, (k, rel_l2(acts[k], blocks[k]))


@pytest.mark.parametrize("name", ["DiffMa-S/7", "DiffMa-B/7"])
def test_patch7_factory_models_forward_and_training_backward_match_oracle(gpu, name):
    """BASELINE config 1's model on the HIP path (VERDICT r3 missing 6): the `/7` factory entries (reference model.py:636-640) give
    L = 16 tokens at the reference's 28 x 28 latents.  One forward against oracle.model_ref (fp32, rel-L2 <= 1e-3) and one
    `training_losses` backward against fp64 autograd through the oracle (every parameter gradient, rel-L2 <= 5e-3)."""
    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.model import DiffMa_models
    from oracle.model_ref import diffma_forward_ref

    torch.manual_seed(5)
    net = DiffMa_models[name](input_size=28, dt_rank=16, d_state=16)
    _rerandomize(net, 6)
    depth = len(net.blocks)
    L, B = 16, 2
    g = torch.Generator().manual_seed(7)
    x, y, y2 = torch.randn(B, 4, 28, 28, generator=g), torch.randn(B, 512, generator=g), torch.randn(B, L, 512, generator=g)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g))
    t = torch.tensor([437, 12])
    nz = torch.randn(B, 4, 28, 28, generator=g)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert net.x_embedder.num_patches == L
    ref = diffma_forward_ref(sd, x, t, y, y2, w, patch_size=7, depth=depth, dtype=torch.float32)
    net = net.to(gpu).train()
    with torch.no_grad():
        out = net(x.to(gpu), t.to(gpu), y=y.to(gpu), y2=y2.to(gpu), w=w.to(gpu)).cpu()
    assert float(ref.abs().mean()) > 1e-3
    assert rel_l2(out, ref) <= 1e-3, rel_l2(out, ref)

    d = create_diffusion("")
    loss = d.training_losses(net, x.to(gpu), t.to(gpu), dict(y=y.to(gpu), y2=y2.to(gpu), w=w.to(gpu)), noise=nz.to(gpu))["loss"].mean()
    loss.backward()
    got = {k: p.grad.detach().cpu().double() for k, p in net.named_parameters() if p.grad is not None}
    sd64 = {k: v.double().clone().requires_grad_(k != "pos_embed") for k, v in sd.items()}
    model = lambda xx, tt, **kws: diffma_forward_ref(sd64, xx, tt, kws["y"], kws["y2"], kws["w"], patch_size=7, depth=depth, dtype=torch.float64)
    ref_loss = d.training_losses(model, x.double(), t, dict(y=y.double(), y2=y2.double(), w=w.double()), noise=nz.double())["loss"].mean()
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 2e-3 * abs(float(ref_loss.detach()))
    for k, gr in got.items():
        r = rel_l2(gr, sd64[k].grad)
        assert r <= 5e-3, (k, r)
    assert len(got) == sum(1 for k in sd64 if k != "pos_embed")


@pytest.mark.parametrize("rms", [True, False])
def test_mamba_split_conv1d_scan_combined_runs_on_the_matrix_pipe(gpu, monkeypatch, rms):
    """Route A of INTEGRATION.md for Mamba-2: the reference-facing operator (block/mamba2.py:392-410) at the DiffMa-XL/2 mixer
    width (d_inner 1024, 16 heads of 64, d_state 16) in bf16 must reach csrc/ssd.hip / csrc/ssd_bwd.hip (no scan launch), with
    and without the gated RMSNorm; output and every gradient against fp64 autograd through the oracle restatement."""
    from diffma_amd import hip_ops
    from diffma_amd.selective_scan_interface import mamba_split_conv1d_scan_combined
    from oracle.mamba2_ref import mamba_split_conv1d_scan_combined_ref

    calls = {"ssd_fwd": 0, "ssd_bwd": 0, "scan_fwd": 0, "scan_bwd": 0}
    for name in calls:
        real = getattr(hip_ops, name)
        monkeypatch.setattr(hip_ops, name, (lambda real, name: lambda *a, **k: (calls.__setitem__(name, calls[name] + 1), real(*a, **k))[1])(real, name))
    gen = torch.Generator().manual_seed(21)
    B, L, H, P, N, dm = 2, 196, 16, 64, 16, 512
    dim = H * P
    mk = lambda *s, sc=1.0: torch.randn(*s, generator=gen) * sc
    zx = mk(B, L, 2 * dim + 2 * N + H).bfloat16()
    cw, cb = mk(dim + 2 * N, 4, sc=0.4), mk(dim + 2 * N, sc=0.1)
    dt_bias, A, D = mk(H, sc=0.5), -(torch.rand(H, generator=gen) * 4 + 0.5), mk(H)
    nw, ow = 1 + mk(dim, sc=0.1), mk(dm, dim, sc=dim ** -0.5)
    dy = mk(B, L, dm)
    kw = dict(chunk_size=256, seq_idx=None, activation="silu", rmsnorm_eps=1e-5, outproj_bias=None, headdim=P, ngroups=1, norm_before_gate=False)
    leaves = [t.to(gpu).requires_grad_(True) for t in (zx, cw, cb, dt_bias, A, D, nw, ow)]
    got = mamba_split_conv1d_scan_combined(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], D=leaves[5],
                                           rmsnorm_weight=leaves[6] if rms else None, outproj_weight=leaves[7].bfloat16(), **kw)
    (got.float() * dy.to(gpu)).sum().backward()
    assert calls == {"ssd_fwd": 1, "ssd_bwd": 1, "scan_fwd": 0, "scan_bwd": 0}, calls
    ref_leaves = [t.float().double().clone().requires_grad_(True) for t in (zx, cw, cb, dt_bias, A, D, nw, ow)]
    ref = mamba_split_conv1d_scan_combined_ref(ref_leaves[0], ref_leaves[1], ref_leaves[2], ref_leaves[3], ref_leaves[4], D=ref_leaves[5],
                                               rmsnorm_weight=ref_leaves[6] if rms else None, outproj_weight=ref_leaves[7], **kw)
    (ref * dy.double()).sum().backward()
    assert got.shape == (B, L, dm) and rel_l2(got.float().cpu(), ref.detach()) <= 2e-2, rel_l2(got.float().cpu(), ref.detach())
    names = ["zxbcdt", "conv_w", "conv_b", "dt_bias", "A", "D", "norm_w", "outproj_w"]
    for k, (a, b) in enumerate(zip(leaves, ref_leaves)):
        if names[k] == "norm_w" and not rms:
            continue
        assert rel_l2(a.grad.float().cpu(), b.grad) <= 4e-2, (names[k], rel_l2(a.grad.float().cpu(), b.grad))


def test_block_passthrough_gradients_equal_autograd_sums(gpu, monkeypatch):
    """The pass-through LayerNorm nodes (block_ops.PASSTHROUGH: the second consumer's gradient is added inside dm_ln_mod_bwd)
    against the same model with autograd's own gradient sums -- including the long skips, where AddBackward hands ONE gradient
    tensor to two nodes (the residual's gradient must only be read): every parameter gradient and the input gradient agree."""
    from diffma_amd import block_ops
    from diffma_amd.diffusion import create_diffusion

    g, sd, net, inp = _g5(gpu)
    net.train()
    d = create_diffusion("")
    z, nz, tt = (torch.from_numpy(g[k]).to(gpu) for k in ("loss_z", "loss_noise", "loss_t"))

    def run(flag):
        monkeypatch.setattr(block_ops, "PASSTHROUGH", flag)
        net.zero_grad(set_to_none=True)
        zz = z.clone().requires_grad_(True)
        loss = d.training_losses(net, zz, tt, dict(y=inp["y"], y2=inp["y2"], w=inp["w"]), noise=nz)["loss"].mean()
        loss.backward()
        return float(loss), zz.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    la, ga, pa = run(True)
    lb, gb, pb = run(False)
    assert la == lb
    torch.testing.assert_close(ga, gb, rtol=1e-5, atol=1e-7)
    assert pa.keys() == pb.keys()
    for k in pa:
        torch.testing.assert_close(pa[k], pb[k], rtol=2e-5, atol=1e-7, msg=lambda m, k=k: f"{k}: {m}")


def test_step_prep_is_bitwise_neutral(gpu, monkeypatch):
    """step_prep.prepare (all mixers' A = -exp(A_log) and the 16-bit weight copies made by a few foreach launches at the top of
    DiffMa.forward) changes launch counts only: loss and every gradient of a bf16-autocast training step are IDENTICAL with and
    without it, and a weight written after prepare() is never served from a stale shadow."""
    from diffma_amd import step_prep
    from diffma_amd.diffusion import create_diffusion

    g, sd, net, inp = _g5(gpu)
    net.train()
    d = create_diffusion("")
    z, nz, tt = (torch.from_numpy(g[k]).to(gpu) for k in ("loss_z", "loss_noise", "loss_t"))

    def run(flag):
        monkeypatch.setattr(step_prep, "ENABLED", flag)
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = d.training_losses(net, z, tt, dict(y=inp["y"], y2=inp["y2"], w=inp["w"]), noise=nz)["loss"].mean()
        loss.backward()
        return float(loss), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    la, pa = run(True)
    lb, pb = run(False)
    assert la == lb and pa.keys() == pb.keys()
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    # staleness: after an in-place update the shadow must not be handed out
    w = net.blocks[0].mamba1.in_proj.weight
    monkeypatch.setattr(step_prep, "ENABLED", True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        step_prep.prepare(net)
    assert step_prep.shadow_of(w, torch.bfloat16) is not None
    with torch.no_grad():
        w.add_(1.0)
    assert step_prep.shadow_of(w, torch.bfloat16) is None
    assert torch.equal(step_prep.cast_weight(w, torch.bfloat16), w.to(torch.bfloat16))
    # id() reuse: an entry left behind by a freed parameter must never serve a new parameter that got its address
    import weakref
    dead = torch.nn.Parameter(torch.zeros(4, 4, device=gpu))
    fresh = torch.nn.Parameter(torch.ones(4, 4, device=gpu))
    step_prep._SHADOWS[id(fresh)] = (weakref.ref(dead), torch.zeros(4, 4, device=gpu, dtype=torch.bfloat16), fresh._version, step_prep._GEN[0])
    assert step_prep.shadow_of(fresh, torch.bfloat16) is None and id(fresh) not in step_prep._SHADOWS


def test_full_width_mixer_takes_the_fused_dtproj_backward(gpu, monkeypatch):
    """At DiffMa's real mixer width (d_model 512 -> d_inner 1024, dt_rank 32) the backward's two dt_proj products come
    from dm_dtproj_bwd (K8b, one read of d delta); every gradient against fp64 autograd through the oracle, and equal (to bf16 rounding)
    to the two-GEMM form (DIFFMA_DTPROJ_BWD_FUSED=0, read by the library at call time)."""
    from diffma_amd import hip_ops
    from diffma_amd.mamba import Mamba
    from diffma_amd.tools import spiral
    from oracle.mamba_ref import mamba_spiral_forward_ref

    calls = {"dtproj_bwd": 0}
    real = hip_ops.dtproj_bwd
    monkeypatch.setattr(hip_ops, "dtproj_bwd", lambda *a, **k: (calls.__setitem__("dtproj_bwd", calls["dtproj_bwd"] + 1), real(*a, **k))[1])
    torch.manual_seed(3)
    n, B, d_model = 4, 8, 512                                       # 3 directions x 8 x 16 tokens = 384 rows
    orders, inverses = spiral(n)
    lists = (orders[2], orders[3], inverses[2], inverses[3])
    mix = Mamba(d_model=d_model, d_state=16, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                origina_list_reversal=lists[3]).to(gpu)
    x0 = torch.randn(B, n * n, d_model, device=gpu)
    dy = torch.randn(B, n * n, d_model, device=gpu)

    def run():
        for p in mix.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mix(x, "spiral")
        (y.float() * dy).sum().backward()
        return y.detach().float(), x.grad.clone(), {k: p.grad.clone() for k, p in mix.named_parameters()}

    y1, dx1, g1 = run()
    assert calls["dtproj_bwd"] == 1, calls
    monkeypatch.setenv("DIFFMA_DTPROJ_BWD_FUSED", "0")
    y0, dx0, g0 = run()
    assert calls["dtproj_bwd"] == 1, calls                        # the predicate said no: the two GEMMs ran
    monkeypatch.delenv("DIFFMA_DTPROJ_BWD_FUSED")
    assert torch.equal(y0, y1)
    assert rel_l2(dx1.cpu(), dx0.cpu()) <= 1e-2
    for k in g1:
        assert rel_l2(g1[k].cpu(), g0[k].cpu()) <= 1e-2, (k, rel_l2(g1[k].cpu(), g0[k].cpu()))
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mix.state_dict().items()}
    x64 = x0.cpu().double().requires_grad_(True)
    yr = mamba_spiral_forward_ref(x64, params, lists, dtype=torch.float64)
    (yr * dy.cpu().double()).sum().backward()
    assert rel_l2(y1.cpu(), yr.detach()) <= 2e-2
    assert rel_l2(dx1.cpu(), x64.grad) <= 6e-2
    for k, g in g1.items():
        assert rel_l2(g.cpu(), params[k].grad) <= 6e-2, (k, rel_l2(g.cpu(), params[k].grad))


def test_small_batch_weight_gradient_gemm_writes_fp32(gpu):
    """Below the split-K threshold the weight-gradient product a^T b leaves the GEMM in fp32 (aten::mm.dtype) instead of as a 16-bit
    result + cast launch: fp32 result, at least as close to the fp64 product as the rounded form."""
    from diffma_amd import projections as proj

    g = torch.Generator().manual_seed(5)
    a = torch.randn(1568, 96, generator=g).bfloat16().to(gpu)
    b = torch.randn(1568, 512, generator=g).bfloat16().to(gpu)
    got = proj._tn_splitk_impl(a, b)
    ref = a.double().t() @ b.double()
    rounded = (a.t() @ b).float()
    assert got.dtype == torch.float32 and got.shape == (96, 512)
    e_new, e_old = rel_l2(got.cpu(), ref.cpu()), rel_l2(rounded.cpu(), ref.cpu())
    assert e_new <= 2e-3 and e_new <= e_old * 1.05, (e_new, e_old)


# ---- the two mixers of a block in one set of launches (reference block/mamba_block.py:107-108; config/brain.yaml: 1 sample / GPU) ----
def test_paired_mixers_equal_two_unpaired_mixers_and_halve_the_launches(gpu, monkeypatch):
    """Spiral_MambaBlock at the reference's own batch (small launches, bf16 autocast): with the pair path the block's two mixers issue
    every stage once (kernels: one grid through the `_n` entry points; projections: batched GEMMs) -- the output and every
    gradient must equal the two-unpaired-mixers form to GEMM rounding, and the mixers' C-ABI launches must halve."""
    import copy

    from diffma_amd import _lib
    from diffma_amd import selective_scan_interface as ssi
    from diffma_amd.mamba_block import Spiral_MambaBlock
    from diffma_amd.tools import spiral

    torch.manual_seed(4)
    n, B, C = 14, 2, 512
    orders, inverses = spiral(n)
    blk0 = Spiral_MambaBlock(C, C, 32, 2 * C, 16, orders[2], orders[3], inverses[2], inverses[3]).to(gpu)
    with torch.no_grad():
        for name, p in blk0.named_parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn_like(p) * 0.02)
    x = torch.randn(B, n * n, C, device=gpu)
    c = torch.randn(B, 2 * C, device=gpu)
    w = torch.sigmoid(torch.randn(B, n * n, 1, device=gpu))
    dy = torch.randn(B, n * n, C, device=gpu)

    def run(pair):
        monkeypatch.setattr(ssi, "PAIR_MIXERS", pair)
        blk = copy.deepcopy(blk0)
        xin = x.clone().requires_grad_(True)
        counts = {"n": 0}
        real_call, real_call_n = _lib.call, _lib.call_n
        monkeypatch.setattr(_lib, "call", lambda name, a, st: (counts.__setitem__("n", counts["n"] + 1), real_call(name, a, st))[1])
        monkeypatch.setattr(_lib, "call_n", lambda name, a, st: (counts.__setitem__("n", counts["n"] + 1), real_call_n(name, a, st))[1])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = blk(xin, c, w)
        (y.float() * dy).sum().backward()
        torch.cuda.synchronize()
        monkeypatch.setattr(_lib, "call", real_call)
        monkeypatch.setattr(_lib, "call_n", real_call_n)
        grads = {k: p.grad.detach().float().clone() for k, p in blk.named_parameters() if p.grad is not None}
        return y.detach().float(), xin.grad.detach().float(), grads, counts["n"]

    y0, dx0, g0, n0 = run(False)
    y1, dx1, g1, n1 = run(True)
    assert rel_l2(y1, y0) <= 1e-2 and rel_l2(dx1, dx0) <= 2e-2, (rel_l2(y1, y0), rel_l2(dx1, dx0))
    assert g0.keys() == g1.keys()
    for k in g0:
        assert rel_l2(g1[k], g0[k]) <= 3e-2, (k, rel_l2(g1[k], g0[k]))
    # block-level kernels (LayerNorms, gate head, blend) are unchanged; the mixers' share of the C-ABI launches halves
    assert n1 < n0 and (n0 - n1) >= 10, (n0, n1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_spiral_pair_equals_two_single_operators_bit_for_bit_on_library_projections(gpu, monkeypatch, dtype):
    """spiral_ssm_pair against spiral_ssm on each mixer alone, with the pair's inner projections on the library (PAIR_OWN_MAX_ROWS 0):
    one operator body serves both, the kernels are bit-identical under the `_n` launches and the library products are the same calls,
    so both outputs and every gradient are EQUAL, and the pair makes fewer C-ABI calls.  spiral(8): L = 64 is the smallest length on
    the chunk-parallel scans; d_model 256 (Din 512, dt_rank 16) the smallest width dm_dtproj_bwd takes."""
    from diffma_amd import _lib
    from diffma_amd import projections as proj
    from diffma_amd import selective_scan_interface as ssi
    from diffma_amd.mamba import Mamba
    from diffma_amd.tools import spiral

    monkeypatch.setattr(proj, "PAIR_OWN_MAX_ROWS", 0)
    torch.manual_seed(7)
    n, B, d_model = 8, 1, 256
    orders, inverses = spiral(n)
    mixers = [Mamba(d_model=d_model, d_state=16, token_list=orders[k], token_list_reversal=orders[k + 1], origina_list=inverses[k],
                    origina_list_reversal=inverses[k + 1]).to(gpu) for k in (2, 4)]
    with torch.no_grad():
        for m in mixers:
            m.D.add_(0.1 * torch.randn_like(m.D))
    assert ssi.spiral_ssm_pair_supported(B, n * n, dtype, *mixers)
    Din = mixers[0].d_inner
    xz = [torch.randn(B, n * n, 2 * Din, device=gpu).to(dtype) for _ in mixers]
    dy = [torch.randn(B, n * n, Din, device=gpu).to(dtype) for _ in mixers]
    names = ("conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "D")

    def run(pair):
        for m in mixers:
            for p in m.parameters():
                p.grad = None
        xin = [t.clone().requires_grad_(True) for t in xz]
        A = [(-torch.exp(m.A_log.detach().float())).requires_grad_(True) for m in mixers]
        counts = {"n": 0}
        real_call, real_call_n = _lib.call, _lib.call_n
        monkeypatch.setattr(_lib, "call", lambda name, a, st: (counts.__setitem__("n", counts["n"] + 1), real_call(name, a, st))[1])
        monkeypatch.setattr(_lib, "call_n", lambda name, a, st: (counts.__setitem__("n", counts["n"] + 1), real_call_n(name, a, st))[1])
        if pair:
            y = ssi.spiral_ssm_pair(xin[0], xin[1], mixers[0], mixers[1], A[0], A[1])
        else:
            y = [ssi.spiral_ssm(x, m.conv1d.weight, m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.dt_proj.bias, a, m.D, m.scan_index)
                 for x, m, a in zip(xin, mixers, A)]
        torch.autograd.backward(list(y), dy)
        torch.cuda.synchronize()
        monkeypatch.setattr(_lib, "call", real_call)
        monkeypatch.setattr(_lib, "call_n", real_call_n)
        got = {}
        for g, m in enumerate(mixers):
            got[f"{g}.y"], got[f"{g}.dxz"], got[f"{g}.dA"] = y[g].detach().clone(), xin[g].grad.clone(), A[g].grad.clone()
            params = dict(m.named_parameters())
            got.update({f"{g}.{k}": params[k].grad.clone() for k in names})
        return got, counts["n"]

    single, n_single = run(False)
    paired, n_paired = run(True)
    assert single.keys() == paired.keys() and len(single) == 2 * 9
    for k in single:
        assert torch.equal(paired[k], single[k]), (k, rel_l2(paired[k].float().cpu(), single[k].float().cpu()))
    assert n_paired < n_single, (n_paired, n_single)


# bounds of the bench-dispatch end-to-end test = 2x the worst case measured on MI355X (profiles/r06_e2e_bench_dispatch_worst.json: output rel-L2
# 3.9e-3; worst parameter gradient 2.04e-2 -- the bias of the fusion MLP's last layer of block 0, a sum over 34 496 bf16 rows)
E2E_OUT_TOL, E2E_GRAD_TOL = 8e-3, 4e-2


def test_bench_dispatch_end_to_end_matches_oracle(gpu, monkeypatch):
    """The composition the bench times, end to end, with NO thresholds patched: a depth-2 DiffMa at the L/2
    width (hidden 512 -> d_inner 1024, dt_rank 32 = hidden / 16, 28 x 28 latents -> L = 196), batch 176 (3 x 176 = 528 sequences >= 512), bf16
    autocast, forward + `training_losses` backward.  At this launch size the library selects K3x (fused conv + x_proj), the K4x slab
    form, the sequential scans K1 / K2, K8 / K8b, the split-K weight gradients and the large-batch projections; the launch log
    below asserts that they are what ran.  Reference arithmetic: fp64 autograd through oracle.model_ref (the fp64 oracle runs ON
    THE DEVICE here, 16 samples at a time -- its sequential scan keeps ~0.6 GB per sample for autograd -- and its parameter
    gradients are summed over the chunks; it is the checker, not the path).  Bounds: output rel-L2 <= 8e-3, every parameter gradient
    rel-L2 <= 4e-2 (bf16 activations, fp32 master weights): twice the measured worst case, which the assert message reports."""
    from diffma_amd import _lib, hip_ops
    from diffma_amd import projections as proj
    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.model import DiffMa
    from oracle.model_ref import diffma_forward_ref

    log = []
    real_call, real_call_n = _lib.call, _lib.call_n

    def call(name, a, st):
        log.append((name, a))
        return real_call(name, a, st)

    def call_n(name, arr, st):
        log.extend((name, a) for a in arr)
        return real_call_n(name, arr, st)

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "call_n", call_n)
    tn = []
    real_tn = proj._tn_splitk_impl
    monkeypatch.setattr(proj, "_tn_splitk_impl", lambda a, b: (tn.append((a.shape[0], a.shape[1], b.shape[1])), real_tn(a, b))[1])

    torch.manual_seed(11)
    depth, B, L = 2, 176, 196
    net = DiffMa(input_size=28, patch_size=2, hidden_size=512, depth=depth, dt_rank=16, d_state=16)
    _rerandomize(net, 12)
    g = torch.Generator().manual_seed(13)
    x, y, y2 = torch.randn(B, 4, 28, 28, generator=g), torch.randn(B, 512, generator=g), torch.randn(B, L, 512, generator=g)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g))
    t = torch.randint(0, 1000, (B,), generator=g)
    nz = torch.randn(B, 4, 28, 28, generator=g)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(gpu).train()
    d = create_diffusion("")
    dev = lambda v: v.to(gpu)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(dev(x), dev(t), y=dev(y), y2=dev(y2), w=dev(w))
        n_fwd = len(log)
        loss = d.training_losses(net, dev(x), dev(t), dict(y=dev(y), y2=dev(y2), w=dev(w)), noise=dev(nz))["loss"].mean()
    del log[:n_fwd]                                            # keep the training step's launches only
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().double() for k, p in net.named_parameters() if p.grad is not None}

    # ---- what ran ------------------------------------------------------------------------------------------------------------
    names = [n for n, _ in log]
    nmix = 2 * depth
    assert names.count("dm_gather_conv1d_xproj_fwd") == nmix, names.count("dm_gather_conv1d_xproj_fwd")          # K3x
    assert names.count("dm_gather_conv1d_xproj_bwd") == nmix                                                     # K4x ...
    lib = _lib.load()
    import ctypes
    for n, a in log:
        if n == "dm_gather_conv1d_xproj_bwd":
            assert a.batch == B and a.ndir == 3 and lib.dm_gather_conv1d_xproj_bwd_slab(ctypes.byref(a), None) > 0   # ... in its slab form
        if n in ("dm_selective_scan_fwd", "dm_selective_scan_bwd"):
            # the library's rule (csrc/scan_fwd_chunked.h use_chunked_fwd, scan_bwd_chunked.h): more than 512 channel-waves -> sequential
            assert a.nseq == 3 * B and a.nseq * ((a.dim + 63) // 64) > 512 and not (a.flags & _lib.DM_FLAG_SCAN_CHUNKED)
    assert names.count("dm_selective_scan_fwd") == nmix and names.count("dm_selective_scan_bwd") == nmix          # K1, K2
    assert names.count("dm_dtproj_softplus_fwd") == nmix and names.count("dm_dtproj_bwd") == nmix                 # K8, K8b
    assert "dm_gather_conv1d_fwd" not in names and "dm_gather_conv1d_bwd" not in names                            # not the unfused pair
    assert "dm_gemm" not in names                                                                                 # not the small-launch GEMM
    # the wide projections on K12 (csrc/gemm_large.hip): in_proj forward and the input gradient of out_proj of every mixer, M = B L rows
    assert sum(1 for n, a in log if n == "dm_gemm_large" and a.P == B * L) >= 2 * nmix, names.count("dm_gemm_large")
    # split-K weight gradients over M = B L rows (in_proj, out_proj, the fusion MLP) and 3 B L rows (x_proj)
    assert sum(1 for m, _, _ in tn if m == B * L) >= 2 * nmix and sum(1 for m, _, _ in tn if m == 3 * B * L) == nmix, tn

    # ---- the oracle, fp64, on the device, 16 samples at a time ------------------------------------------------------------------
    sd64 = {k: v.double().to(gpu).requires_grad_(k != "pos_embed") for k, v in sd.items()}
    model = lambda xx, tt, **kws: diffma_forward_ref(sd64, xx, tt, kws["y"], kws["y2"], kws["w"], patch_size=2, depth=depth, dtype=torch.float64)
    ref_out, ref_loss = [], 0.0
    for i in range(0, B, 16):
        s = slice(i, i + 16)
        c = lambda v: v[s].double().to(gpu)
        with torch.no_grad():
            ref_out.append(model(c(x), dev(t[s]), y=c(y), y2=c(y2), w=c(w)))
        part = d.training_losses(model, c(x), dev(t[s]), dict(y=c(y), y2=c(y2), w=c(w)), noise=c(nz))["loss"].sum() / B
        part.backward()
        ref_loss += float(part.detach())
    ref_out = torch.cat(ref_out).detach()
    assert float(ref_out.abs().mean()) > 1e-3
    assert rel_l2(out.detach().float().cpu(), ref_out.cpu()) <= E2E_OUT_TOL, rel_l2(out.detach().float().cpu(), ref_out.cpu())
    assert abs(float(loss.detach()) - ref_loss) <= 1e-2 * abs(ref_loss), (float(loss.detach()), ref_loss)
    worst = {}
    for k, gr in got.items():
        worst[k] = rel_l2(gr.cpu(), sd64[k].grad.cpu())
    wk = max(worst, key=worst.get)
    rep = os.environ.get("DIFFMA_TEST_REPORT_DIR")
    if rep:                                                    # measured worst cases of this run (tools/r06_gpu_checks.sh keeps them under profiles/)
        import json
        with open(os.path.join(rep, "e2e_bench_dispatch_worst.json"), "w") as f:
            json.dump({"out_rel_l2": rel_l2(out.detach().float().cpu(), ref_out.cpu()), "worst_grad": [wk, worst[wk]],
                       "grads_rel_l2": dict(sorted(worst.items(), key=lambda kv: -kv[1])[:12])}, f, indent=1)
    bad = {k: v for k, v in worst.items() if not v <= E2E_GRAD_TOL}
    assert not bad, f"{len(bad)} gradients above {E2E_GRAD_TOL}: {bad}; worst of all {wk} = {worst[wk]:.3e}"
    assert len(got) == sum(1 for k in sd64 if k != "pos_embed")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mamba_inner_fn_reference_call_pattern_at_large_launch(gpu, dtype):
    """INTEGRATION route A in the dispatch a large batch takes: mamba_inner_fn on a CrossScan slice with 512 sequences per call
    (block/mamba.py:343-348) -- dm_repack in, the fused conv + x_proj kernels, ONE direction with the gate and the softplus hoisted
    out of the sequential scans, dx / dz written straight into d(xz), dm_repack out -- forward and every gradient against fp64
    autograd through the oracle's mamba_inner_ref."""
    from diffma_amd import hip_ops
    from diffma_amd.selective_scan_interface import mamba_inner_fn
    from oracle.mamba_ref import mamba_inner_ref

    gen = torch.Generator().manual_seed(11)
    B, Din, L, N, R, dm = 512, 128, 28, 16, 32, 64          # dt_rank 32: x_proj has the 64 rows the fused conv + x_proj backward is built for
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc)
    xs = mk(B, 3, 2 * Din, L).to(dtype)
    cw, cb = mk(Din, 1, 4, sc=0.5), mk(Din, sc=0.1)
    xw, dw, ow = mk(R + 2 * N, Din, sc=0.1).to(dtype), mk(Din, R, sc=0.3).to(dtype), mk(dm, Din, sc=0.1).to(dtype)
    A, Dp, bias = -(torch.rand(Din, N, generator=gen) * 3 + 0.2), mk(Din), mk(Din, sc=0.3)
    go = mk(B, L, dm).to(dtype)
    names = "xs conv_w conv_b x_proj dt_proj out_proj A D dt_bias".split()
    host = [xs, cw, cb, xw, dw, ow, A, Dp, bias]
    dev = [t.to(gpu).requires_grad_(True) for t in host]
    log = []
    timer_was = hip_ops._TIMER

    class _Log:
        def launch(self, name, nbytes, fn, design_bytes=None, flops=0):
            log.append(name)
            fn()

    hip_ops.set_timer(_Log())
    try:
        x_, cw_, cb_, xw_, dw_, ow_, A_, D_, b_ = dev
        o = mamba_inner_fn(x_[:, 1], cw_, cb_, xw_, dw_, ow_, None, A_, None, None, D_, delta_bias=b_, delta_softplus=True)
        (o.float() * go.to(gpu).float()).sum().backward()
        torch.cuda.synchronize()
    finally:
        hip_ops.set_timer(timer_was)
    assert log.count("dm_repack") == 2, log
    if dtype == torch.bfloat16:          # the large-launch dispatch: fused conv + x_proj both ways, hoisted gate, no copy passes
        assert "dm_gather_conv1d_xproj_fwd" in log and "dm_gather_conv1d_xproj_bwd" in log and "dm_gate_bwd" in log, log
        assert log.count("dm_token_merge") == 1, log          # the gate pass of the forward; no dx / dz copy passes in the backward
    ref = [t.double().requires_grad_(True) for t in host]
    x_, cw_, cb_, xw_, dw_, ow_, A_, D_, b_ = ref
    ro = mamba_inner_ref(x_[:, 1], cw_, cb_, xw_, dw_, ow_, None, A_, None, None, D_, delta_bias=b_, delta_softplus=True)
    (ro * go.double()).sum().backward()
    tol_o, tol_g = {torch.bfloat16: (1e-2, 3e-2), torch.float32: (1e-4, 5e-4)}[dtype]
    assert rel_l2(o.detach().float().cpu(), ro.detach()) <= tol_o
    assert float(dev[0].grad[:, 0].abs().max()) == 0.0 and float(dev[0].grad[:, 2].abs().max()) == 0.0      # the other slices get no gradient
    for a, b, name in zip(dev, ref, names):
        assert rel_l2(a.grad.float().cpu(), b.grad) <= tol_g, (name, rel_l2(a.grad.float().cpu(), b.grad))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_route_a_model_equals_native_model(gpu, dtype):
    """INTEGRATION route A at model level: the reference's own Mamba.forward structure -- channel-major xz, CrossScan buffer, three
    mamba_inner_fn calls on its strided slices, output buffer, CrossMerge (block/mamba.py:333-355), as bench.py --route-a restates
    it -- gives the same training loss and the same parameter gradients as the native fused 3-direction mixer on the same weights
    (fp32: <= 1e-4 / 1e-3; bf16 autocast: both are 16-bit evaluations of the same function, <= 2e-2 / 8e-2)."""
    import bench
    from diffma_amd import selective_scan_interface as ssi
    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.mamba import Mamba
    from diffma_amd.model import DiffMa

    torch.manual_seed(21)
    net = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=4, d_state=16)
    _rerandomize(net, 22)
    net = net.to(gpu).train()
    B, L = 3, 16
    g = torch.Generator().manual_seed(23)
    x, y, y2 = torch.randn(B, 4, 8, 8, generator=g).to(gpu), torch.randn(B, 64, generator=g).to(gpu), torch.randn(B, L, 64, generator=g).to(gpu)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g)).to(gpu)
    t = torch.randint(0, 1000, (B,), generator=g).to(gpu)
    nz = torch.randn(B, 4, 8, 8, generator=g).to(gpu)
    d = create_diffusion("")

    def run():
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            loss = d.training_losses(net, x, t, dict(y=y, y2=y2, w=w), noise=nz)["loss"].mean()
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: p.grad.detach().double().cpu() for k, p in net.named_parameters() if p.grad is not None}

    loss_b, grads_b = run()
    fwd, pair = Mamba.forward, ssi.PAIR_MIXERS
    try:
        bench.install_route_a()
        assert Mamba.forward is not fwd
        loss_a, grads_a = run()
    finally:
        Mamba.forward, ssi.PAIR_MIXERS = fwd, pair
    tol_l, tol_g = {torch.float32: (1e-4, 1e-3), torch.bfloat16: (2e-2, 8e-2)}[dtype]
    assert abs(loss_a - loss_b) <= tol_l * abs(loss_b), (loss_a, loss_b)
    assert grads_a.keys() == grads_b.keys()
    bad = {k: rel_l2(grads_a[k], grads_b[k]) for k in grads_b if float(grads_b[k].norm()) > 0 and not rel_l2(grads_a[k], grads_b[k]) <= tol_g}
    assert not bad, bad


def test_adaln_of_all_blocks_in_one_product_equals_per_block(gpu, monkeypatch):
    """mamba_block.adaln_all: the 16-bit adaLN weights of all blocks are the rows of one buffer (step_prep) and every block's
    (shift, scale, gate) comes from ONE product (reference: each block applies adaLN_modulation to the same c, block/mamba_block.py:
    82-85, 101) -- same loss and the same gradient for every parameter (incl. each block's adaLN weight / bias, handed back as row
    views of one product) as the per-block products, in the bf16 autocast step; a second step after an optimizer update still agrees
    (the stacked copies are refreshed by prepare())."""
    import copy

    from diffma_amd import mamba_block
    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.model import DiffMa

    torch.manual_seed(31)
    net0 = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=4, d_state=16)
    _rerandomize(net0, 32)
    B, L = 3, 16
    g = torch.Generator().manual_seed(33)
    x, y, y2 = torch.randn(B, 4, 8, 8, generator=g).to(gpu), torch.randn(B, 64, generator=g).to(gpu), torch.randn(B, L, 64, generator=g).to(gpu)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g)).to(gpu)
    t = torch.randint(0, 1000, (B,), generator=g).to(gpu)
    nz = torch.randn(B, 4, 8, 8, generator=g).to(gpu)
    d = create_diffusion("")
    used = []
    real = mamba_block._AdaLNAllFn.apply
    monkeypatch.setattr(mamba_block._AdaLNAllFn, "apply", staticmethod(lambda *a: (used.append(1), real(*a))[1]))

    def run(flag):
        monkeypatch.setattr(mamba_block, "ADALN_ALL", flag)
        net = copy.deepcopy(net0).to(gpu).train()
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0)
        out = []
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = d.training_losses(net, x, t, dict(y=y, y2=y2, w=w), noise=nz)["loss"].mean()
            loss.backward()
            out.append((float(loss.detach()), {k: p.grad.detach().double().cpu() for k, p in net.named_parameters() if p.grad is not None}))
            opt.step()
        return out

    ref = run(False)
    assert not used
    got = run(True)
    assert len(used) == 2
    for (la, ga), (lb, gb) in zip(got, ref):
        assert abs(la - lb) <= 5e-3 * abs(lb), (la, lb)
        assert ga.keys() == gb.keys()
        bad = {k: rel_l2(ga[k], gb[k]) for k in gb if float(gb[k].norm()) > 0 and not rel_l2(ga[k], gb[k]) <= 3e-2}
        assert not bad, bad
        assert all(k in ga for k in gb if "adaLN_modulation" in k)
