"""dm_gemm_large with its gated epilogue (gate_z set) against the unfused pair it replaces, per element, and the mixer backward with the switch on and off.

The calls go through the C ABI with hand-built structs.  The REFERENCE for g and dz is dm_gemm_large followed by dm_gate_bwd at the same
inputs (tests/test_gate_in_dgrad_cpu.py has the case builder and the shape table).  The epilogue rounds the accumulator to the I/O dtype
before it gates, so g and dz must come out BIT-IDENTICAL to that pair, in bf16 and in fp16; the comparison runs on the device over all
P x 1024 elements.  g = (dy z) sg is a chain of products and is held to that without exception.  dz contains 1 + z (1 - sg), which is
open to contraction into an FMA, and the compiler decides per instantiation (tests/test_mixer_passes_gpu.py meets the same between two
instantiations of dm_gate_bwd): where dz differs, `_finish` prints the count and holds EVERY element of the fused g and dz to the
dm_gate_bwd bounds of tests/test_mixer_passes_cpu.py against fp64, on the pair's own 16-bit dy -- no other tolerance exists here.
On the MI355X when this file was written: bf16 bit-identical in every case; fp16 g bit-identical, dz differing in 268 of 16 777 216
elements of the one-round case, each by one unit in the last place, all of them the odd element of a pair, nearly all at z around -1.28
(where 1 + z (1 - sg) cancels), and every element within its bound.

Outputs are NaN-filled views inside sentinel frames: in the xz layout z and dz are the RIGHT halves of [P, 2048] buffers (the left half
of d(xz) is frame), contiguous otherwise.  dy_tail, where a remainder needs it, is a view in a frame as well; where none is passed no dy
buffer exists at all.
"""
import pytest
import torch

from tests.test_block_ops_gpu import _ok, _raw
from tests.test_gate_in_dgrad_cpu import Q, ROUND, SHAPES, TAIL, gated_args, gated_case
from tests.test_mixer_passes_cpu import BF16, CODE, DM_ERR_ARG, DM_ERR_DTYPE, DM_ERR_LAYOUT, F16, NAN, NS, bits_equal, gate_bwd_eval

pytestmark = pytest.mark.gpu

SENT = 7.0
_CASES = {}


def _case(gpu, dt, P, Kc):
    """Inputs on the device and the unfused pair's (dy, g, dz), made once per (dtype, P, Kc) and left unchanged."""
    key = (dt, P, Kc)
    if key not in _CASES:
        from diffma_amd._lib import dm_gate_bwd_args, dm_gemm_args

        c = gated_case(dt, P, Kc, seed=P + Kc)
        d = NS(c=c, a=c.a.to(gpu), b=c.b.to(gpu), z=c.z.to(gpu), pre=c.pre.to(gpu))
        d.dy, d.g, d.dz = (torch.full((P, Q), NAN, dtype=dt, device=gpu) for _ in range(3))
        m = dm_gemm_args()
        m.P, m.Q, m.Kc, m.ab_dtype, m.c_dtype, m.a_kmajor, m.b_kmajor = P, Q, Kc, CODE[dt], CODE[dt], 1, 1
        m.a, m.b, m.c, m.lda, m.ldb, m.ldc = d.a.data_ptr(), d.b.data_ptr(), d.dy.data_ptr(), Kc, Kc, Q
        _ok("dm_gemm_large", m)
        gb = dm_gate_bwd_args()
        gb.batch, gb.seqlen, gb.dim, gb.io_dtype = 1, P, Q, CODE[dt]
        gb.dy, gb.z, gb.pre, gb.g, gb.dz = d.dy.data_ptr(), d.z.data_ptr(), d.pre.data_ptr(), d.g.data_ptr(), d.dz.data_ptr()
        gb.dy_sl = gb.z_sl = gb.p_sl = gb.g_sl = gb.dz_sl = Q
        _ok("dm_gate_bwd", gb)
        torch.cuda.synchronize()
        assert not bool(d.dy.isnan().any())
        _CASES.clear()                                           # one case resident at a time
        _CASES[key] = d
    return _CASES[key]


def _framed(gpu, dt, P, half, fill=None):
    """[P, Q] view in a sentinel frame: the right half of a [P + 4, 2 Q] buffer (xz layout), or rows of Q with two spare rows either side."""
    ld = 2 * Q if half else Q
    buf = torch.full((P + 4, ld), SENT, dtype=dt, device=gpu)
    view = buf[2:2 + P, ld - Q:]
    if fill is None:
        view.fill_(NAN)
    else:
        view.copy_(fill)
    assert view.data_ptr() % 16 == 0 and view.stride() == (ld, 1)
    return buf, view


def _intact(buf, view, what):
    chk = buf.clone()
    chk.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(SENT)
    assert bool((chk == SENT).all()), f"{what}: written outside its view"


def _build(gpu, d, half, tail):
    c = d.c
    m = NS(d=d)
    m.zbuf, m.z = _framed(gpu, c.dt, c.P, half, d.z)
    m.gbuf, m.g = _framed(gpu, c.dt, c.P, False)
    m.dzbuf, m.dz = _framed(gpu, c.dt, c.P, half)
    m.tbuf = m.tail = None
    if tail:
        m.tbuf = torch.full((tail + 4, Q + 8), SENT, dtype=c.dt, device=gpu)
        m.tail = m.tbuf[2:2 + tail, :Q]
        m.tail.fill_(NAN)
    m.a = gated_args(c.P, Q, c.Kc, CODE[c.dt], d.a.data_ptr(), d.b.data_ptr(), m.z.data_ptr(), d.pre.data_ptr(), m.g.data_ptr(),
                     m.dz.data_ptr(), dy_tail=m.tail.data_ptr() if tail else 0, ldz=m.z.stride(0), lddz=m.dz.stride(0),
                     ld_tail=Q + 8 if tail else Q)
    return m


def _compare(d, name, got, want):
    """Bit for bit on the device; a difference is counted, printed and then held to the dm_gate_bwd bounds against fp64."""
    it = torch.int16
    diff = got.contiguous().view(it) != want.view(it)
    n = int(diff.sum())
    print(f"gate_in_dgrad {name}: {n} of {want.numel()} elements differ from the unfused pair")
    return n


def _finish(gpu, m):
    torch.cuda.synchronize()
    d = m.d
    _intact(m.gbuf, m.g, "g")
    _intact(m.dzbuf, m.dz, "dz")
    _intact(m.zbuf, m.z, "z")
    if m.tbuf is not None:
        _intact(m.tbuf, m.tail, "dy_tail")
    ng, ndz = _compare(d, "g", m.g, d.g), _compare(d, "dz", m.dz, d.dz)
    assert ng == 0, "g = (dy z) sg is a chain of products: nothing to contract, it must equal the pair bit for bit"
    if ndz:
        # the last place of dz where the two kernels' 1 + z (1 - sg) contract differently: every element of the fused g and dz is
        # held to the dm_gate_bwd bounds against fp64, on the 16-bit dy the unfused pair stored
        c = d.c
        gate_bwd_eval(NS(dt=c.dt, dy=d.dy.cpu(), z=c.z, pre=c.pre), m.g.cpu(), m.dz.cpu(), book={}, op="gate_in_dgrad")
    return ndz


LAYOUTS = [("xz", True), ("contig", False)]


@pytest.mark.parametrize("lay,half", LAYOUTS, ids=[n for n, _ in LAYOUTS])
@pytest.mark.parametrize("name,P,Kc", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_gated_equals_gemm_large_then_gate_bwd(gpu, dt, name, P, Kc, lay, half):
    """One whole round of tiles; the round plus 300 rows (the remainder takes dm_gemm + dm_gate_bwd: the seam is compared like any
    other row); a contraction of two 16-step groups; a remainder large enough to stay in the persistent kernel, ending in a row block
    of 156 rows; and K = 64, which K12 does not take: dm_gemm_large refuses it with and without the gated epilogue and write nothing."""
    from diffma_amd import _lib

    if Kc % 512:
        c = gated_case(dt, 2048, Kc, seed=1)
        d = NS(c=NS(dt=dt, P=P, Kc=Kc), a=torch.zeros(P, Kc, dtype=dt, device=gpu), b=c.b.to(gpu),
               z=torch.zeros(P, Q, dtype=dt, device=gpu), pre=torch.zeros(P, Q, dtype=dt, device=gpu))
        m = _build(gpu, d, half, 0)
        assert _raw("dm_gemm_large", m.a) == DM_ERR_ARG
        plain = _lib.dm_gemm_args()
        plain.P, plain.Q, plain.Kc, plain.ab_dtype, plain.c_dtype, plain.a_kmajor, plain.b_kmajor = P, Q, Kc, CODE[dt], CODE[dt], 1, 1
        plain.a, plain.b, plain.c, plain.lda, plain.ldb, plain.ldc = d.a.data_ptr(), d.b.data_ptr(), m.g.data_ptr(), Kc, Kc, Q
        assert _raw("dm_gemm_large", plain) == DM_ERR_ARG
        torch.cuda.synchronize()
        assert bool(m.g.isnan().all()) and bool(m.dz.isnan().all())
        return
    tail = int(_lib.load().dm_gemm_large_tail_rows(P, Q))
    assert tail == TAIL[name]
    m = _build(gpu, _case(gpu, dt, P, Kc), half, tail)
    _ok("dm_gemm_large", m.a)
    ndz = _finish(gpu, m)
    assert dt == F16 or ndz == 0, f"bf16 dz differs from the unfused pair in {ndz} elements (it did not when this test was written)"


def test_gated_refusals_leave_the_outputs_alone(gpu):
    """On real buffers: fp32, a pointer off its 16-byte boundary, a width that is no multiple of the row piece, strides that differ
    between z and dz, and a remainder without its dy slice."""
    dt, P = BF16, ROUND + 300
    c = NS(dt=dt, P=P, Kc=512)
    d = NS(c=c, a=torch.zeros(P, 512, dtype=dt, device=gpu), b=torch.zeros(Q, 512, dtype=dt, device=gpu),
           z=torch.zeros(P, Q, dtype=dt, device=gpu), pre=torch.zeros(P, Q, dtype=dt, device=gpu))
    for kw, want in [(dict(ab_dtype=0, c_dtype=0), DM_ERR_DTYPE), (dict(a_by=2), DM_ERR_LAYOUT), (dict(gate_z_by=8), DM_ERR_LAYOUT),
                     (dict(gate_g_by=2), DM_ERR_LAYOUT), (dict(gate_dz_by=4), DM_ERR_LAYOUT), (dict(Q=1000), DM_ERR_ARG),
                     (dict(Q=1028), DM_ERR_ARG), (dict(gate_lddz=Q), DM_ERR_LAYOUT), (dict(c=0), DM_ERR_ARG), (dict(Kc=64), DM_ERR_ARG)]:
        m = _build(gpu, d, True, 300)
        for k, v in kw.items():
            if k.endswith("_by"):
                setattr(m.a, k[:-3], getattr(m.a, k[:-3]) + v)
            else:
                setattr(m.a, k, v)
        assert _raw("dm_gemm_large", m.a) == want, kw
        torch.cuda.synchronize()
        assert bool(m.g.isnan().all()) and bool(m.dz.isnan().all()) and bool(m.tail.isnan().all()), kw


def test_block_backward_is_the_same_with_the_switch_on_and_off(gpu, monkeypatch):
    """One DiffMa block at the smallest size that takes K12 for out_proj's input gradient: hidden 512 (d_inner 1024) and 171 samples
    of 196 tokens -- 3 x 171 = 513 sequences per mixer is where the large-launch path begins (hip_ops.XPROJ_FUSED_MIN_SEQS; below it
    the two mixers share their launches and keep the gate pass), 33 516 rows = two rounds of tiles and 748 rows for the small-launch
    kernel.  Forward + backward under bf16 autocast with the switch on and off: the fused run records dm_gemm_large_gated twice and no
    dm_gate_bwd of the full size (only the remainders'), the other one no dm_gemm_large_gated, and the output, both input gradients and
    every parameter gradient are bit-identical.  (bf16 is the dtype in which the kernel pair is bit-identical; what flows from an fp16
    dz that differs in a last place has no bound function of its own.)"""
    from diffma_amd import _lib, hip_ops
    from diffma_amd.mamba_block import Spiral_MambaBlock
    from diffma_amd.tools import spiral

    torch.manual_seed(0)
    dt, hidden, n, B = BF16, 512, 14, 171
    assert 3 * B >= hip_ops.XPROJ_FUSED_MIN_SEQS > 3 * (B - 1)
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
    names, real = [], _lib.call
    gated = lambda name, a: "dm_gemm_large_gated" if (name == "dm_gemm_large" and a.gate_z) else name      # (the flag form of the entry)
    monkeypatch.setattr(_lib, "call", lambda name, a, st: (names.append(gated(name, a)), real(name, a, st))[1])

    def run(on):
        monkeypatch.setattr(hip_ops, "GATE_IN_DGRAD", on)
        del names[:]
        blk.zero_grad(set_to_none=True)
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dt):
            y = blk(x, c, w)
        (y.float() * dy).sum().backward()
        torch.cuda.synchronize()
        return list(names), [y.detach(), x.grad, c.grad] + [p.grad.clone() for _, p in sorted(blk.named_parameters())]

    n_on, r_on = run(True)
    n_off, r_off = run(False)
    assert n_on.count("dm_gemm_large_gated") == 2, n_on
    assert n_off.count("dm_gemm_large_gated") == 0 and n_off.count("dm_gate_bwd") == 2, n_off
    keys = ["y", "x.grad", "c.grad"] + [k for k, _ in sorted(blk.named_parameters())]
    for k, a, b in zip(keys, r_on, r_off):
        assert a is not None and b is not None, k
        assert bits_equal(a, b), f"{k}: the switch changes the result"
