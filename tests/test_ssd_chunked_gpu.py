"""dm_ssd_fwd_chunked (csrc/ssd_chunked.hip) on the GPU: per element against fp64 within the bound of tests/test_ssd_chunked_cpu.py
(read its docstring first), and what goes with it: no-grad Mamba-2 calls past L = 224 take the chunked entry at the widths of
hip_ops.SSD_FWD_CHUNKED_WIDTHS, calls that need gradients the A-shared scan pair, nothing changes at L <= 224, and the drop-in operator
no longer refuses chunk_size < L.

Buffers as in tests/test_ssd_wide_gpu._run_case: x | B | C are column blocks of one NaN-padded buffer, out is a view inside a sentinel
frame that starts as NaN.  The reference and the bound of a case are computed once on the host (analysis, cached).  The lengths are
those of the CPU file, by name: Q is the chunk length the library reports for the width (2 Q and 256 coincide where Q = 128).
"""
import ctypes

import pytest
import torch

from tests.test_ssd_chunked_cpu import MAXL, analysis, chunk_len, inputs
from tests.test_ssd_gpu import A_H, BF16, BIAS_H, D_H, DM_ERR_ARG, F16, NAME, NAN, P, SENT, _ratio
from tests.test_ssd_wide_cpu import head_params
from tests.test_ssd_wide_gpu import _logged

pytestmark = pytest.mark.gpu

LENGTH = {"Q+1": lambda Q: Q + 1, "2Q": lambda Q: 2 * Q, "2Q+33": lambda Q: 2 * Q + 33, "256": lambda Q: 256, "1024": lambda Q: MAXL,
          "1": lambda Q: 1, "33": lambda Q: 33, "Q": lambda Q: Q}


def _launch(gpu, c, N, nh, dtype, gate_pad=0, entry="ssd_fwd_chunked", gate=True):
    """Device buffers of the case and one launch: (framed buffer, out view, operand buffers and their copies).  gate False: z = None."""
    from diffma_amd import hip_ops

    L, S, din = c["L"], c["S"], nh * P
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
    out = getattr(hip_ops, entry)(x, Bm, Cm, c["dt_tok"].to(gpu), z if gate else None, A, D, bias, out=view, z_row_index=c["zperm"].int().to(gpu),
                                  out_row_index=c["operm"].int().to(gpu), batch_per_dir=c["bpd"])
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    return buf, view, (xb, xb0, zb, zb0)


def _run_case(gpu, L, dtype, N, nh=4, gate_pad=0, family="randn", gate=True):
    """One launch of hip_ops.ssd_fwd_chunked: every element of out within the bound, the frame around out bit for bit, the operands
    unchanged.  gate False: the launch gets z = None and is held to the reference and the bound of the operator without a gate."""
    c = inputs(L, dtype, N, nh, family)
    ref, tol = analysis(L, dtype, N, nh, family, gate)
    S, din = c["S"], nh * P
    buf, view, (xb, xb0, zb, zb0) = _launch(gpu, c, N, nh, dtype, gate_pad, gate=gate)
    chk = buf.clone()
    chk[:, 2:2 + L, :din] = SENT
    assert bool((chk == SENT).all()), "written outside out"
    assert torch.equal(xb.view(torch.int16), xb0.view(torch.int16)) and torch.equal(zb.view(torch.int16), zb0.view(torch.int16)), "operands are read-only"
    r = _ratio(view.cpu().reshape(S, L, din), ref, tol)
    worst = float(r.max())
    per_head = [round(float(r.reshape(S, L, nh, P)[:, :, h].max()), 3) for h in range(nh)]
    print(f"worst |got - ref| / bound  out N {N} {NAME[dtype]} L {L} heads {nh} {family}{'' if gate else ' no gate'}: {worst:.4f}")
    assert worst <= 1.0, f"out N {N} {NAME[dtype]} L {L} {family}: worst |got - ref| / bound {worst:.3f}; per head {per_head}"


@pytest.mark.parametrize("length", ["Q+1", "2Q", "2Q+33", "256", "1024"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N", [16, 128])
def test_ssd_fwd_chunked_within_derived_bound(gpu, N, dtype, length):
    """d_state 16 and 128 at every length of the CPU file: four heads in the four regimes, per element within the bound."""
    _run_case(gpu, LENGTH[length](chunk_len(N)), dtype, N)


@pytest.mark.parametrize("length", ["Q+1", "2Q+33"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N", [32, 64])
def test_ssd_fwd_chunked_middle_widths_within_derived_bound(gpu, N, dtype, length):
    """d_state 32 and 64 one token past a chunk and at three chunks with a ragged last one."""
    _run_case(gpu, LENGTH[length](chunk_len(N)), dtype, N)


@pytest.mark.parametrize("length", ["2Q+33", "1024"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N", [16, 128])
def test_ssd_fwd_chunked_coherent_rows_within_derived_bound(gpu, N, dtype, length):
    """The coherent family (what the state carries adds up): the inputs on which an overwritten or undecayed carry is 27 bounds away."""
    _run_case(gpu, LENGTH[length](chunk_len(N)), dtype, N, family="coherent")


@pytest.mark.parametrize("length", ["1", "33", "Q"])
def test_ssd_fwd_chunked_single_chunk(gpu, length):
    """Short sequences are one chunk of the new entry: d_state 128, bf16."""
    _run_case(gpu, LENGTH[length](chunk_len(128)), BF16, 128)


@pytest.mark.parametrize("nh", [2, 3, 16])
def test_ssd_fwd_chunked_head_counts(gpu, nh):
    """Head counts that leave a workgroup with surplus waves across the chunk loop (2, 3) and that take several workgroups per sequence
    (16): d_state 128, bf16, L = 2 Q + 33; the regimes are cycled over the heads."""
    _run_case(gpu, 2 * chunk_len(128) + 33, BF16, 128, nh)


@pytest.mark.parametrize("N", [16, 128])
def test_ssd_fwd_chunked_gate_rows_on_4_byte_boundaries(gpu, N):
    """The gate of a two-head mixer starts its rows on 4-byte boundaries only; the chunked entry takes that at every width."""
    _run_case(gpu, 2 * chunk_len(N) + 33, BF16, N, 2, gate_pad=2)


@pytest.mark.parametrize("N", [16, 128])
def test_ssd_fwd_chunked_without_gate(gpu, N):
    """dm_ssd_fwd_chunked with z = NULL, the arm no other kernel-level test reaches: d_state 16 and 128, bf16, L = Q + 1 (a full
    chunk and one token that reads the carried state), three heads.  Reference: the fp64 dual form with out = Y + D x; bound:
    tests.test_ssd_chunked_cpu.chunked_bound without the gate's factor and error term."""
    _run_case(gpu, chunk_len(N) + 1, BF16, N, 3, gate=False)


def test_ssd_fwd_chunked_is_deterministic(gpu):
    """Two launches on the same operands agree bit for bit (d_state 128, bf16, L = 2 Q + 33)."""
    N = 128
    c = inputs(2 * chunk_len(N) + 33, BF16, N)
    a = _launch(gpu, c, N, 4, BF16)[1].clone()
    b = _launch(gpu, c, N, 4, BF16)[1].clone()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_ssd_fwd_chunked_c_abi_refuses_1025_and_the_single_chunk_entry_225(gpu):
    """dm_ssd_fwd_args built by hand: seqlen 1025 returns DM_ERR_ARG from dm_ssd_fwd_chunked and writes nothing; dm_ssd_fwd still
    returns DM_ERR_ARG at 225; the same struct at 225 runs through the chunked entry."""
    from diffma_amd import _lib

    lib = _lib.load()
    N, nh, S = 16, 1, 1
    din = nh * P
    g = torch.Generator().manual_seed(5)
    mk = lambda L: dict(x=torch.randn(S, L, din, generator=g).to(BF16).to(gpu), B=torch.randn(S, L, N, generator=g).to(BF16).to(gpu),
                        C=torch.randn(S, L, N, generator=g).to(BF16).to(gpu), dt=(torch.randn(S, L, nh, generator=g) - 3).to(BF16).to(gpu),
                        out=torch.full((S, L, din), SENT, dtype=BF16, device=gpu))
    A = torch.tensor([-1.0], device=gpu)

    def args(t, L):
        a = _lib.dm_ssd_fwd_args()
        a.nseq, a.batch_per_dir, a.seqlen, a.nheads, a.headdim, a.dstate = S, 0, L, nh, P, N
        a.io_dtype, a.flags = _lib.DM_BF16, 0
        a.x, a.B, a.C, a.dt, a.z, a.A, a.out = t["x"].data_ptr(), t["B"].data_ptr(), t["C"].data_ptr(), t["dt"].data_ptr(), None, A.data_ptr(), t["out"].data_ptr()
        a.x_ss, a.x_sl, a.B_ss, a.B_sl, a.C_ss, a.C_sl = L * din, din, L * N, N, L * N, N
        a.dt_sb, a.dt_sl, a.o_ss, a.o_sl = L * nh, nh, L * din, din
        return a

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = mk(1025)
    assert lib.dm_ssd_fwd_chunked(ctypes.byref(args(t, 1025)), stream) == DM_ERR_ARG
    torch.cuda.synchronize()
    assert bool((t["out"] == SENT).all())
    t = mk(225)
    assert lib.dm_ssd_fwd(ctypes.byref(args(t, 225)), stream) == DM_ERR_ARG
    torch.cuda.synchronize()
    assert bool((t["out"] == SENT).all())
    assert lib.dm_ssd_fwd_chunked(ctypes.byref(args(t, 225)), stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t["out"].float()).all()) and not bool((t["out"] == SENT).all())


# =====================================================================================================================================
# routing, mixer, operator, model
# =====================================================================================================================================
@pytest.mark.parametrize("N", [16, 128])
def test_long_no_grad_calls_take_the_chunked_entry_and_training_the_scan_pair(gpu, monkeypatch, N):
    """spiral_ssd at L = 256, two directions: without gradients it launches dm_ssd_fwd_chunked and no scan; with gradients the A-shared
    scan pair and nothing of dm_ssd*, finite gradients, and the two outputs agree at the tolerance of tests/test_ssd_wide_gpu.py; with
    the width left out of hip_ops.SSD_FWD_CHUNKED_WIDTHS, or hip_ops.SSD_CHUNKED off, the no-grad call is back on the scan; at L = 196
    the no-grad call still launches dm_ssd_fwd."""
    from diffma_amd import hip_ops
    from diffma_amd import selective_scan_interface as ssi

    monkeypatch.setattr(hip_ops, "SSD_FWD_CHUNKED_WIDTHS", (16, 32, 64, 128))
    monkeypatch.setattr(hip_ops, "SSD_CHUNKED", True)
    log = _logged(monkeypatch)
    Hm, Bsz = 8, 1
    Din = Hm * P
    Cx = Din + 2 * N
    g = torch.Generator().manual_seed(300 + N)
    conv_w, conv_b = (torch.randn(Cx, 4, generator=g) * 0.3).to(gpu), (torch.randn(Cx, generator=g) * 0.1).to(gpu)
    par = [A_H.float().repeat(2).to(gpu), D_H.float().repeat(2).to(gpu), BIAS_H.float().repeat(2).to(gpu), torch.ones(Din, device=gpu)]

    def case(L):
        zx = (torch.randn(Bsz, L, 2 * Din + 2 * N + Hm, generator=g) * 0.5).to(BF16).to(gpu)
        idx = torch.stack([torch.arange(L), torch.randperm(L, generator=g)]).int().to(gpu)
        inv = torch.argsort(idx.long(), dim=1).int()
        return zx, (lambda zin: ssi.spiral_ssd(zin, conv_w, conv_b, par[2], par[0], par[1], par[3], 1e-5, idx, inv, Din, N))

    zx, run = case(256)
    del log[:]
    with torch.no_grad():
        y0 = run(zx)
    torch.cuda.synchronize()
    assert "dm_ssd_fwd_chunked" in log and "dm_selective_scan_fwd" not in log and "dm_ssd_fwd" not in log, log
    del log[:]
    zg = zx.clone().requires_grad_(True)
    y1 = run(zg)
    y1.backward(torch.ones_like(y1))
    torch.cuda.synchronize()
    assert "dm_selective_scan_fwd" in log and "dm_selective_scan_bwd" in log and not [n for n in log if n.startswith("dm_ssd")], log
    assert bool(torch.isfinite(zg.grad.float()).all())
    torch.testing.assert_close(y1.float(), y0.float(), rtol=3e-2, atol=5e-2 * max(1.0, float(y0.float().abs().max())))
    for name, value in (("SSD_FWD_CHUNKED_WIDTHS", ()), ("SSD_CHUNKED", False)):
        del log[:]
        with monkeypatch.context() as m:
            m.setattr(hip_ops, name, value)
            with torch.no_grad():
                run(zx)
            torch.cuda.synchronize()
        assert "dm_selective_scan_fwd" in log and "dm_ssd_fwd_chunked" not in log, (name, log)
    zx, run = case(196)
    del log[:]
    with torch.no_grad():
        run(zx)
    torch.cuda.synchronize()
    assert "dm_ssd_fwd" in log and "dm_ssd_fwd_chunked" not in log and "dm_selective_scan_fwd" not in log, log


def test_mamba2_mixer_at_256_tokens_no_grad_on_the_chunked_entry(gpu, monkeypatch):
    """Mamba2(d_model=64) (two heads, default d_state 128) on the spiral lists of a 16 x 16 grid under bf16 autocast and no_grad: the
    call runs dm_ssd_fwd_chunked and is within rel-L2 2e-2 of mamba2_spiral_forward_ref in fp64 (the bound of
    test_mamba2_mixer_wide_no_grad_on_the_matrix_pipe for this mixer)."""
    from diffma_amd import hip_ops
    from diffma_amd.mamba2 import Mamba2
    from oracle.mamba2_ref import mamba2_spiral_forward_ref
    from tests.test_dstate_gpu import _spiral_lists
    from tests.test_model_gpu import rel_l2

    monkeypatch.setattr(hip_ops, "SSD_FWD_CHUNKED_WIDTHS", (16, 32, 64, 128))
    monkeypatch.setattr(hip_ops, "SSD_CHUNKED", True)
    log = _logged(monkeypatch)
    torch.manual_seed(9)
    n = 16
    lists = _spiral_lists(n, 4)
    mix = Mamba2(d_model=64, d_conv=4, expand=2, token_list=lists[0], token_list_reversal=lists[1], origina_list=lists[2],
                 origina_list_reversal=lists[3]).to(gpu)
    assert mix.d_state == 128 and mix.nheads == 2
    with torch.no_grad():
        mix.norm.weight.add_(torch.randn_like(mix.norm.weight) * 0.1)
        mix.D.add_(torch.randn_like(mix.D) * 0.1)
    x = torch.randn(2, n * n, 64, device=gpu)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = mix(x, "spiral")
    torch.cuda.synchronize()
    assert "dm_ssd_fwd_chunked" in log and "dm_selective_scan_fwd" not in log, log
    params = {k: v.detach().cpu().double() for k, v in mix.state_dict().items()}
    yr = mamba2_spiral_forward_ref(x.cpu().double(), params, lists, headdim=64, dtype=torch.float64)
    err = rel_l2(y.float().cpu(), yr)
    print(f"Mamba2(d_model=64) L 256 no-grad rel-L2 {err:.3e}")
    assert err <= 2e-2, err


def test_mamba_split_conv1d_scan_combined_takes_chunk_size_below_seqlen(gpu, monkeypatch):
    """The drop-in operator at L = 256 (16 heads of 64, d_state 16, bf16, no gradients): chunk_size 64 and chunk_size 256 give the same
    tensor bit for bit (the kernel's own chunk length applies), through dm_ssd_fwd_chunked, within rel-L2 2e-2 of the fp64 restatement
    (the tolerance of test_mamba_split_conv1d_scan_combined_runs_on_the_matrix_pipe)."""
    from diffma_amd import hip_ops
    from diffma_amd.selective_scan_interface import mamba_split_conv1d_scan_combined
    from oracle.mamba2_ref import mamba_split_conv1d_scan_combined_ref
    from tests.test_model_gpu import rel_l2

    monkeypatch.setattr(hip_ops, "SSD_FWD_CHUNKED_WIDTHS", (16, 32, 64, 128))
    monkeypatch.setattr(hip_ops, "SSD_CHUNKED", True)
    log = _logged(monkeypatch)
    gen = torch.Generator().manual_seed(31)
    B, L, H, N, dm = 2, 256, 16, 16, 512
    dim = H * P
    mk = lambda *s, sc=1.0: torch.randn(*s, generator=gen) * sc
    zx = mk(B, L, 2 * dim + 2 * N + H).bfloat16()
    cw, cb = mk(dim + 2 * N, 4, sc=0.4), mk(dim + 2 * N, sc=0.1)
    dt_bias, A, D = mk(H, sc=0.5), -(torch.rand(H, generator=gen) * 4 + 0.5), mk(H)
    nw, ow = 1 + mk(dim, sc=0.1), mk(dm, dim, sc=dim ** -0.5)
    kw = dict(seq_idx=None, activation="silu", rmsnorm_eps=1e-5, outproj_bias=None, headdim=P, ngroups=1, norm_before_gate=False)
    dev = [t.to(gpu) for t in (zx, cw, cb, dt_bias, A, D, nw, ow)]
    got = {}
    with torch.no_grad():
        for cs in (64, 256):
            got[cs] = mamba_split_conv1d_scan_combined(dev[0], dev[1], dev[2], dev[3], dev[4], D=dev[5], chunk_size=cs, rmsnorm_weight=dev[6],
                                                       outproj_weight=dev[7].bfloat16(), **kw)
    torch.cuda.synchronize()
    assert log.count("dm_ssd_fwd_chunked") == 2 and "dm_selective_scan_fwd" not in log, log
    assert torch.equal(got[64].view(torch.int16), got[256].view(torch.int16))
    ref = mamba_split_conv1d_scan_combined_ref(*(t.float().double() for t in (zx, cw, cb, dt_bias, A)), D=D.double(), chunk_size=256,
                                               rmsnorm_weight=nw.double(), outproj_weight=ow.double(), **kw)
    err = rel_l2(got[64].float().cpu(), ref)
    print(f"mamba_split_conv1d_scan_combined L 256 rel-L2 {err:.3e}")
    assert got[64].shape == (B, L, dm) and err <= 2e-2, err


def test_tiny_diffma_mamba2_at_256_tokens_samples_on_the_chunked_entry(gpu, monkeypatch):
    """The tiny DiffMa(input_size=32, patch_size=2, use_mamba2=True, d_state=128) (256 tokens) in eval mode under bf16 autocast: the
    eager call launches dm_ssd_fwd_chunked and is finite, and one hipGraph replay of the denoiser is bit-equal to it."""
    from diffma_amd import hip_ops
    from diffma_amd.graphed import GraphedDenoiser
    from diffma_amd.model import DiffMa
    from tests.test_model_gpu import _rerandomize

    monkeypatch.setattr(hip_ops, "SSD_FWD_CHUNKED_WIDTHS", (16, 32, 64, 128))
    monkeypatch.setattr(hip_ops, "SSD_CHUNKED", True)
    torch.manual_seed(21)
    net = DiffMa(input_size=32, patch_size=2, hidden_size=64, depth=2, use_mamba2=True, d_state=128)
    _rerandomize(net, 22)
    L, B = 256, 2
    g = torch.Generator().manual_seed(23)
    x, y, y2 = torch.randn(B, 4, 32, 32, generator=g), torch.randn(B, 64, generator=g), torch.randn(B, L, 64, generator=g)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g))
    t = torch.tensor([437, 12])
    net = net.to(gpu).eval()
    x, y, y2, w, t = (v.to(gpu) for v in (x, y, y2, w, t))
    log = _logged(monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        eager = net(x, t, y=y, y2=y2, w=w)
    torch.cuda.synchronize()
    assert "dm_ssd_fwd_chunked" in log, log
    assert bool(torch.isfinite(eager.float()).all()) and float(eager.float().abs().mean()) > 1e-3
    gd = GraphedDenoiser(net, x, t, y, y2, w, autocast_dtype=torch.bfloat16, snapshot_weights=False)
    torch.testing.assert_close(gd(x, t, y=y, y2=y2, w=w).clone(), eager, rtol=0, atol=0)
