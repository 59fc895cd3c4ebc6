"""dm_ssd_fwd at the wide states (d_state 32, 64, 128) on the GPU: per element against fp64 within the forward bound of
tests/test_ssd_gpu.py with the state width as a parameter (tests/test_ssd_wide_cpu.py restates it: K0 = 72 + 2 (N - 16) + 2 (l + 1)),
and the dispatch that goes with it: no-grad Mamba-2 calls take the matrix pipe at the widths of hip_ops.SSD_FWD_WIDTHS, calls that
need gradients take the A-shared scan pair (dm_ssd_bwd is d_state 16 only).

Buffers as there: x | B | C are column blocks of one NaN-padded buffer, out is a view inside a sentinel frame that starts as NaN.
The reference and the bound of a case are computed once on the host (tests.test_ssd_wide_cpu.analysis, cached).
"""
import pytest
import torch

from tests.test_ssd_gpu import A_H, BF16, BIAS_H, D_H, F16, NAME, NAN, P, SENT, _ratio
from tests.test_ssd_wide_cpu import WIDTHS, analysis, head_params, inputs

pytestmark = pytest.mark.gpu

GPU_L = [1, 31, 32, 33, 65, 97, 196, 224]


def _lib():
    from diffma_amd import _lib as L

    return L


def _run_case(gpu, L, dtype, N, nh=4, gate_pad=0, gate=True):
    """One launch of hip_ops.ssd_fwd on the case (L, dtype, N, nh): every element of out within the bound, the frame around out
    bit for bit, the operands unchanged.  gate_pad: spare columns behind every row of z (2: rows on 4-byte boundaries only).
    gate False: the launch gets z = None and is held to the reference and the bound of the operator without a gate."""
    from diffma_amd import hip_ops

    c = inputs(L, dtype, N, nh)
    ref, tol = analysis(L, dtype, N, nh, gate)
    S, din = c["S"], nh * P
    xb = torch.full((S, L + 4, din + 2 * N + 8), NAN, dtype=dtype, device=gpu)           # NaN rows before / after, NaN columns beside
    xb[:, 2:2 + L, :din + 2 * N] = c["xBC"].to(gpu)
    v = xb[:, 2:2 + L]
    x, Bm, Cm = v[..., :din], v[..., din:din + N], v[..., din + N:din + 2 * N]
    zb = torch.full((c["bpd"], L, din + gate_pad), NAN, dtype=dtype, device=gpu)
    zb[..., :din] = c["z"].to(gpu)
    z = zb[..., :din]
    xb0, zb0 = xb.clone(), zb.clone()
    buf = torch.full((S, L + 4, din + 8), SENT, dtype=dtype, device=gpu)
    view = buf[:, 2:2 + L, :din]
    view.fill_(NAN)
    A, D, bias = (t.float().to(gpu) for t in head_params(nh))
    out = hip_ops.ssd_fwd(x, Bm, Cm, c["dt_tok"].to(gpu), z if gate else None, A, D, bias, out=view, z_row_index=c["zperm"].int().to(gpu),
                          out_row_index=c["operm"].int().to(gpu), batch_per_dir=c["bpd"])
    torch.cuda.synchronize()
    chk = buf.clone()
    chk[:, 2:2 + L, :din] = SENT
    assert out.data_ptr() == view.data_ptr() and bool((chk == SENT).all()), "written outside out"
    assert torch.equal(xb.view(torch.int16), xb0.view(torch.int16)) and torch.equal(zb.view(torch.int16), zb0.view(torch.int16)), "operands are read-only"
    r = _ratio(view.cpu().reshape(S, L, din), ref, tol)
    worst = float(r.max())
    per_head = [round(float(r.reshape(S, L, nh, P)[:, :, h].max()), 3) for h in range(nh)]
    print(f"worst |got - ref| / bound  out N {N} {NAME[dtype]} L {L} heads {nh}{'' if gate else ' no gate'}: {worst:.4f}")
    assert worst <= 1.0, f"out N {N} {NAME[dtype]} L {L}: worst |got - ref| / bound {worst:.3f}; per head {per_head}"


@pytest.mark.parametrize("L", GPU_L)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N", WIDTHS)
def test_ssd_fwd_wide_within_derived_bound(gpu, N, dtype, L):
    """dm_ssd_fwd at d_state N per element within the forward bound; four heads in the four regimes, the directions and batches of FWD_L."""
    _run_case(gpu, L, dtype, N)


@pytest.mark.parametrize("nh", [2, 3, 16])
def test_ssd_fwd_wide_head_counts(gpu, nh):
    """A workgroup serves four heads: two and three heads leave it with surplus waves, sixteen take four workgroups per sequence.
    d_state 128, bf16, L = 65; the regimes are cycled over the heads."""
    _run_case(gpu, 65, BF16, 128, nh)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_ssd_fwd_wide_gate_rows_on_4_byte_boundaries(gpu, dtype):
    """The gate of a two-head mixer is a view of in_proj rows of 2 Din + 2 N + 2 elements: its rows start on 4-byte boundaries only,
    which the wide kernel reads as dwords.  Same bound; d_state 128, two heads, L = 65 and 33."""
    for L in (65, 33):
        _run_case(gpu, L, dtype, 128, 2, gate_pad=2)


@pytest.mark.parametrize("N", [16, 128])
def test_ssd_fwd_without_gate(gpu, N):
    """dm_ssd_fwd with z = NULL, the arm no other kernel-level test reaches: d_state 16 (ssd_fwd_kernel) and 128 (the wide kernel),
    bf16, L = 33 (two tiles, the second ragged), three heads (one surplus head in the wide workgroup).  Reference: the fp64 dual form
    with out = Y + D x; bound: tests.test_ssd_wide_cpu.fwd_bound without the gate's factor and error term."""
    _run_case(gpu, 33, BF16, N, 3, gate=False)


def _logged(monkeypatch):
    L_ = _lib()
    log, real = [], L_.call
    monkeypatch.setattr(L_, "call", lambda name, a, st: (log.append(name), real(name, a, st))[1])
    return log


def test_wide_no_grad_calls_take_the_matrix_pipe_and_training_the_scan_pair(gpu, monkeypatch):
    """For every routed width beyond 16: spiral_ssd without gradients launches dm_ssd_fwd and no scan; the same call with gradients
    launches the A-shared scan pair and nothing of dm_ssd (there is no wide backward), its gradients are finite, and the two
    outputs agree at the tolerance of test_kernels_gpu.py.  With hip_ops.SSD_MFMA off the no-grad call is back on the scan."""
    from diffma_amd import hip_ops
    from diffma_amd import selective_scan_interface as ssi

    assert 128 in hip_ops.SSD_FWD_WIDTHS
    log = _logged(monkeypatch)
    Hm, L, Bsz = 8, 65, 1
    Din = Hm * P
    for N in [n for n in hip_ops.SSD_FWD_WIDTHS if n > 16]:
        Cx = Din + 2 * N
        g = torch.Generator().manual_seed(200 + N)
        zx = (torch.randn(Bsz, L, 2 * Din + 2 * N + Hm, generator=g) * 0.5).to(BF16).to(gpu)
        conv_w, conv_b = (torch.randn(Cx, 4, generator=g) * 0.3).to(gpu), (torch.randn(Cx, generator=g) * 0.1).to(gpu)
        idx = torch.stack([torch.arange(L), torch.randperm(L, generator=g)]).int().to(gpu)
        inv = torch.argsort(idx.long(), dim=1).int()
        par = [A_H.float().repeat(2).to(gpu), D_H.float().repeat(2).to(gpu), BIAS_H.float().repeat(2).to(gpu), torch.ones(Din, device=gpu)]
        run = lambda zin: ssi.spiral_ssd(zin, conv_w, conv_b, par[2], par[0], par[1], par[3], 1e-5, idx, inv, Din, N)
        del log[:]
        with torch.no_grad():
            y0 = run(zx)
        torch.cuda.synchronize()
        assert "dm_ssd_fwd" in log and "dm_selective_scan_fwd" not in log, (N, log)
        del log[:]
        zg = zx.clone().requires_grad_(True)
        y1 = run(zg)
        y1.backward(torch.ones_like(y1))
        torch.cuda.synchronize()
        assert "dm_selective_scan_fwd" in log and "dm_selective_scan_bwd" in log and not [n for n in log if n.startswith("dm_ssd")], (N, log)
        assert bool(torch.isfinite(zg.grad.float()).all())
        torch.testing.assert_close(y1.float(), y0.float(), rtol=3e-2, atol=5e-2 * max(1.0, float(y0.float().abs().max())))
        del log[:]
        with monkeypatch.context() as m:
            m.setattr(hip_ops, "SSD_MFMA", False)
            with torch.no_grad():
                run(zx)
            torch.cuda.synchronize()
        assert "dm_selective_scan_fwd" in log and "dm_ssd_fwd" not in log, (N, log)


@pytest.mark.parametrize("d_state", [64, None], ids=["64", "default-128"])
def test_mamba2_mixer_wide_no_grad_on_the_matrix_pipe(gpu, monkeypatch, d_state):
    """Mamba2(d_model=64) (two heads) with d_state 64 and with its default of 128 under bf16 autocast and no_grad, against
    mamba2_spiral_forward_ref in fp64 at the bf16 forward bound of test_mamba2_mixer_wide (2e-2 rel-L2); the call runs dm_ssd_fwd."""
    from diffma_amd.mamba2 import Mamba2
    from oracle.mamba2_ref import mamba2_spiral_forward_ref
    from tests.test_dstate_gpu import _spiral_lists
    from tests.test_model_gpu import rel_l2

    log = _logged(monkeypatch)
    torch.manual_seed(9)
    n = 4
    lists = _spiral_lists(n, 4)
    kw = {} if d_state is None else dict(d_state=d_state)
    mix = Mamba2(d_model=64, d_conv=4, expand=2, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                 origina_list_reversal=lists[3], **kw).to(gpu)
    assert mix.d_state == (128 if d_state is None else d_state) and mix.nheads == 2
    with torch.no_grad():
        mix.norm.weight.add_(torch.randn_like(mix.norm.weight) * 0.1)
        mix.D.add_(torch.randn_like(mix.D) * 0.1)
    x = torch.randn(2, n * n, 64, device=gpu)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = mix(x, "spiral")
    torch.cuda.synchronize()
    assert "dm_ssd_fwd" in log and "dm_selective_scan_fwd" not in log, log
    params = {k: v.detach().cpu().double() for k, v in mix.state_dict().items()}
    yr = mamba2_spiral_forward_ref(x.cpu().double(), params, lists, headdim=64, dtype=torch.float64)
    assert rel_l2(y.float().cpu(), yr) <= 2e-2, rel_l2(y.float().cpu(), yr)


def test_tiny_diffma_mamba2_default_width_samples_on_the_matrix_pipe(gpu, monkeypatch):
    """The tiny DiffMa(use_mamba2=True, d_state=128) of test_tiny_diffma_wide_forward_training_backward_and_graph in eval mode under
    bf16 autocast: the eager call launches dm_ssd_fwd, and one hipGraph replay of the denoiser is bit-equal to it."""
    from diffma_amd.graphed import GraphedDenoiser
    from diffma_amd.model import DiffMa
    from tests.test_model_gpu import _rerandomize

    torch.manual_seed(21)
    net = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=4, use_mamba2=True, d_state=128)
    _rerandomize(net, 22)
    L, B = 16, 2
    g = torch.Generator().manual_seed(23)
    x, y, y2 = torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 64, generator=g), torch.randn(B, L, 64, generator=g)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g))
    t = torch.tensor([437, 12])
    net = net.to(gpu).eval()
    x, y, y2, w, t = (v.to(gpu) for v in (x, y, y2, w, t))
    log = _logged(monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        eager = net(x, t, y=y, y2=y2, w=w)
    torch.cuda.synchronize()
    assert "dm_ssd_fwd" in log, log
    assert bool(torch.isfinite(eager.float()).all()) and float(eager.float().abs().mean()) > 1e-3
    gd = GraphedDenoiser(net, x, t, y, y2, w, autocast_dtype=torch.bfloat16, snapshot_weights=False)
    torch.testing.assert_close(gd(x, t, y=y, y2=y2, w=w).clone(), eager, rtol=0, atol=0)
