"""GPU parity of the chunk-parallel forward scan past one segment (csrc/scan_fwd_chunked.h: 196 < L <= 1024, the sequence walked in
segments of G = 14 waves x 14 steps with the state carried between them) against the fp64 oracle, on inputs where the state
remembers (a wrong carry is invisible where it has decayed to 1e-10).  The same inputs through the sequential kernel must stay
inside the same bounds in the same test.  Tolerances are those of tests/test_kernels_gpu.py.
"""
import functools

import pytest
import torch

from tests.test_kernels_gpu import TOL, _ckpt_states, _inputs_long_memory, _oracle_states

pytestmark = pytest.mark.gpu

BSZ, NDIR, N = 2, 3, 16
S = BSZ * NDIR
NW = 14                        # waves per workgroup = chunks per segment
ONE = 196                      # up to here a launch is one segment (the kernel as it was)


def _G():
    from diffma_amd import hip_ops

    g = hip_ops.scan_fwd_segment(S, 128, 256, N, 0)
    assert g > 0, "a 6-sequence, 128-channel launch at 256 tokens must take the chunk-parallel forward"
    return g


def _len(spec):
    """A length is a number of tokens, or (g, c, k) = g segments + c wave chunks + k tokens of the long form's geometry as the library
    reports it: (1, 0, 1) is G + 1."""
    if isinstance(spec, int):
        return spec
    g, c, k = spec
    return g * _G() + c * (_G() // NW) + k


@functools.lru_cache(maxsize=None)
def _case(dtype, L, Dm, pattern):
    """Host inputs and the fp64 reference of one case, computed once: per-sequence outputs [S][L, Dm] in scan order and the state
    after every step of the first and the last sequence.  pattern: "gated" (z through row indices, softplus in the scan), "ashared"
    (the same with one decay per channel), "hoisted" (no z, delta already activated: what the sampler launches)."""
    from oracle.mamba_ref import selective_scan_ref

    host, _ = _inputs_long_memory(S, L, Dm, N, dtype, seed=L + Dm, dev="cpu", with_z=False, a_shared=pattern == "ashared")
    g = torch.Generator().manual_seed(9)
    zsrc = torch.randn(BSZ, L, Dm, generator=g).to(dtype) if pattern != "hoisted" else None
    perms = torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(NDIR - 1)]).int()
    operms = torch.stack([torch.randperm(L, generator=g) for _ in range(NDIR)]).int()
    ohost = host
    if pattern == "hoisted":
        # the kernel is handed act = softplus(delta + bias) rounded to the I/O dtype; the oracle takes it back through softplus^-1 in
        # fp32 (relative error 4e-7 in dt, far below every bound here), so the imported oracles apply unchanged
        act = torch.nn.functional.softplus(host["delta"].double() + host["bias"].double()).to(dtype)
        host = dict(host, act=act)
        ohost = dict(host, delta=torch.log(torch.expm1(act.double())).float(), bias=torch.zeros(Dm))
    refs = []
    for s in range(S):
        k, b = divmod(s, BSZ)
        cm = lambda t: t[s:s + 1].float().permute(0, 2, 1).double()
        zz = None if zsrc is None else zsrc[b][perms[k].long()].float().T[None].double()
        ref = selective_scan_ref(cm(ohost["u"]), cm(ohost["delta"]), ohost["A"].double(), cm(ohost["B"]), cm(ohost["C"]), ohost["D"].double(),
                                 z=zz, delta_bias=ohost["bias"].double(), delta_softplus=True)
        refs.append(ref[0].T.contiguous())
    states = {s: _oracle_states(ohost, s) for s in (0, S - 1)}
    return host, zsrc, perms, operms, refs, states


def _run(gpu, case, pattern, variant, with_ckpt=True, bc_fp32=False):
    from diffma_amd import hip_ops

    host, zsrc, perms, operms, _, _ = case
    dev = lambda t: None if t is None else t.to(gpu)
    u = dev(host["u"])
    _, L, Dm = u.shape
    Bm, Cm = (dev(host[k].float() if bc_fp32 else host[k]) for k in ("B", "C"))
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, u.dtype, gpu).zero_() if with_ckpt else None
    kw = dict(z_row_index=dev(perms), out_row_index=dev(operms), batch_per_dir=BSZ, ckpt=ckpt, variant=variant)
    if pattern == "hoisted":
        out = hip_ops.scan_fwd(u, dev(host["act"]), dev(host["A"]), Bm, Cm, dev(host["D"]), None, dev(host["bias"]), True, delta_activated=True, **kw)
    else:
        out = hip_ops.scan_fwd(u, dev(host["delta"]), dev(host["A"]), Bm, Cm, dev(host["D"]), dev(zsrc), dev(host["bias"]), True,
                               a_shared=pattern == "ashared", **kw)
    torch.cuda.synchronize()
    return out, ckpt


def _worst(case, out, ckpt):
    """(worst output error, worst state error), each as a fraction of its bound: outputs TOL with atol * max(1, max|ref|); states
    rtol 1e-4, atol 1e-5 max(1, max|h|) for fp32 checkpoints and u |h| + (1 + u) x that, u = 2^-8, for packed bf16 ones."""
    from diffma_amd import hip_ops

    _, _, _, operms, refs, states = case
    rtol, atol = TOL[out.dtype]
    o = out.float().cpu().double()
    L, Dm = o.shape[1:]
    wo = 0.0
    for s in range(S):
        ref = refs[s]
        bound = atol * max(1.0, float(ref.abs().max())) + rtol * ref.abs()
        wo = max(wo, float(((o[s][operms[s // BSZ].long()] - ref).abs() / bound).max()))
    wh = 0.0
    if ckpt is not None:
        K = hip_ops.SCAN_CKPT_EVERY
        got_h = _ckpt_states(ckpt, N, Dm).cpu().double()
        for s, hs in states.items():
            for c in range(hip_ops.scan_nchunk(L, K)):
                want = hs[(c * K if c else L) - 1].T
                tol32 = 1e-4 * want.abs() + 1e-5 * max(1.0, float(want.abs().max()))
                tol = tol32 if ckpt.dtype != torch.int32 else 2.0 ** -8 * want.abs() + (1 + 2.0 ** -8) * tol32
                wh = max(wh, float(((got_h[s, c] - want).abs() / tol).max()))
    return wo, wh


def _check(gpu, dtype, L, Dm, pattern, **kw):
    case = _case(dtype, L, Dm, pattern)
    fig = {}
    for variant in ("sequential", "chunked"):
        out, ckpt = _run(gpu, case, pattern, variant, **kw)
        fig[variant] = _worst(case, out, ckpt)
        print(f"scan_fwd {pattern} {dtype} L {L} Dm {Dm} {variant}: worst error / bound  out {fig[variant][0]:.3f}  states {fig[variant][1]:.3f}")
    assert max(fig["sequential"]) <= 1.0, ("the sequential kernel leaves the bound", fig)
    assert max(fig["chunked"]) <= 1.0, fig
    return case


FP32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16


@pytest.mark.parametrize("dtype,L", [
    (FP32, (1, 0, 1)), (BF16, (1, 0, 1)), (FP16, (1, 0, 1)), (FP32, (1, 1, 1)), (FP32, (2, 0, 0)), (FP32, (2, 0, 1)),
    (FP32, 256), (BF16, 256), (FP16, 256), (FP32, 1024),
    (FP32, 197), (BF16, 197), (FP16, 197), (FP32, (2, 1, 1)), (FP32, (3, 0, 1))],
    ids=["fp32-G+1", "bf16-G+1", "fp16-G+1", "fp32-G+LC+1", "fp32-2G", "fp32-2G+1", "fp32-256", "bf16-256", "fp16-256", "fp32-1024",
         "fp32-197", "bf16-197", "fp16-197", "fp32-2G+LC+1", "fp32-3G+1"])
def test_outputs_and_every_checkpoint_against_fp64(gpu, dtype, L):
    """Gated + softplus through random row-index tables, three directions sharing one z, with checkpoints: outputs of every sequence
    and EVERY checkpoint slot of the first and the last sequence, chunk-parallel and sequential, inside the bounds of _worst.  With
    G the segment length the library reports past 196 tokens (140): 197 is the shortest segmented launch (a second segment with a
    ragged chunk and 8 empty waves), 2G + 1 and 3G + 1 end in a one-token segment (all waves but one empty), 2G + LC + 1 in a ragged
    second chunk, 2G in a full one; G + 1 and G + LC + 1 are below 197 and stay on the one-segment form.  Measured on one MI355X, worst
    error over its bound at 1024 tokens, fp32: sequential 0.15 (outputs) / 0.18 (states), chunk-parallel 0.15 / 0.13; the packed bf16
    checkpoints sit at 0.96 in both kernels (the bound is the format's own rounding)."""
    from diffma_amd import _lib, hip_ops

    L = _len(L)
    assert hip_ops.scan_fwd_segment(S, 128, L, N, _lib.DM_FLAG_SCAN_CHUNKED) == (_G() if L > ONE else ONE)
    _check(gpu, dtype, L, 128, "gated")


@pytest.mark.parametrize("dtype,L,Dm,pattern,kw", [
    (FP32, 256, 200, "gated", {}),                               # ragged channel block
    (FP32, 256, 128, "ashared", {}),                             # one exp per (channel, step), with checkpoints
    (BF16, 256, 128, "ashared", dict(with_ckpt=False)),
    (BF16, 256, 128, "hoisted", dict(with_ckpt=False)),          # the sampler's launch
    (BF16, (2, 0, 1), 128, "hoisted", {}),                           # the same with checkpoints (training under the hoisted softplus)
    (BF16, 256, 128, "gated", dict(bc_fp32=True)),               # bf16 I/O with fp32 B / C
    (FP16, 256, 128, "gated", dict(with_ckpt=False)),            # the generic instantiation
], ids=["dim200", "ashared", "ashared-nockpt", "hoisted", "hoisted-ckpt", "bf16-fp32bc", "nockpt"])
def test_call_patterns(gpu, dtype, L, Dm, pattern, kw):
    _check(gpu, dtype, _len(L), Dm, pattern, **kw)


def test_library_choice_is_the_chunked_kernel_and_is_deterministic(gpu):
    """variant=None (the library's own choice) is bit-equal to variant="chunked" at 256 tokens, run twice; the sequential kernel gives
    other bits, so the comparison can tell them apart."""
    case = _case(FP32, 256, 128, "gated")
    runs = [_run(gpu, case, "gated", v) for v in (None, "chunked", "chunked", "sequential")]
    eq = lambda a, b: torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert eq(runs[0], runs[1]) and eq(runs[1], runs[2])
    assert not torch.equal(runs[0][0].view(torch.int32), runs[3][0].view(torch.int32))


@pytest.mark.parametrize("Bsz,chunked", [(5, True), (6, False)])
def test_checkpoint_launches_are_routed_up_to_256_channel_waves(gpu, Bsz, chunked):
    """Past 196 tokens a launch that writes checkpoints is the library's up to 256 channel-waves (profiles/scan_fwd_chunked_long.json):
    at dim 1024, 15 sequences (240) leave the bits of the chunk-parallel kernel, 18 (288) those of the sequential one."""
    from diffma_amd import hip_ops
    from tests.test_kernels_gpu import _inputs

    L, Dm = 197, 1024
    Sq = 3 * Bsz
    assert hip_ops.scan_fwd_segment(Sq, Dm, L, N, 0) == _G()                 # without checkpoints both sizes are routed
    _, d = _inputs(Sq, L, Dm, N, BF16, seed=Bsz, dev=gpu, with_z=False)
    idx = torch.stack([torch.randperm(L, generator=torch.Generator().manual_seed(k)) for k in range(3)]).int().to(gpu)
    act = torch.nn.functional.softplus(d["delta"].float()).to(BF16)
    got = {}
    for variant in (None, "chunked", "sequential"):
        ckpt = hip_ops.alloc_scan_ckpt(Sq, L, N, Dm, BF16, gpu).zero_()
        out = hip_ops.scan_fwd(d["u"], act, d["A"], d["B"], d["C"], d["D"], None, None, True, delta_activated=True, z_row_index=idx,
                               out_row_index=idx, batch_per_dir=Bsz, ckpt=ckpt, variant=variant)
        got[variant] = (out.view(torch.int16), ckpt)
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not same(got["chunked"], got["sequential"])
    assert same(got[None], got["chunked" if chunked else "sequential"])


def test_pair_is_one_launch_and_bit_equal_to_two(gpu, monkeypatch):
    """Two congruent structs at L 256 through dm_selective_scan_fwd_n, as hip_ops.both issues them: one call, the bits of two."""
    from diffma_amd import _lib, hip_ops

    host, _, perms, operms, _, _ = _case(BF16, 256, 128, "hoisted")
    dev = lambda t: t.to(gpu)
    first = dict(u=dev(host["u"]), act=dev(host["act"]), A=dev(host["A"]), B=dev(host["B"]), C=dev(host["C"]), D=dev(host["D"]),
                 zi=dev(perms), oi=dev(operms))
    ops = [first, dict(first, u=first["u"].flip(0).contiguous(), A=first["A"] * 0.5, B=first["C"], C=first["B"])]     # congruent, other data
    launch = lambda o: hip_ops.scan_fwd(o["u"], o["act"], o["A"], o["B"], o["C"], o["D"], None, None, True, delta_activated=True,
                                        z_row_index=o["zi"], out_row_index=o["oi"], batch_per_dir=BSZ)
    single = [launch(o) for o in ops]
    calls = []
    real_n = _lib.call_n
    monkeypatch.setattr(_lib, "call_n", lambda name, arr, st: (calls.append((name, len(arr))), real_n(name, arr, st))[1])
    pair = hip_ops.both(lambda i: launch(ops[i]))
    torch.cuda.synchronize()
    assert calls == [("dm_selective_scan_fwd", 2)], calls
    assert not torch.equal(single[0], single[1])
    for a, b in zip(single, pair):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_1025_tokens_stay_on_the_sequential_kernel(gpu):
    from diffma_amd import _lib, hip_ops

    L = 1025
    assert hip_ops.scan_fwd_segment(S, 128, L, N, 0) == 0 and hip_ops.scan_fwd_segment(S, 128, L, N, _lib.DM_FLAG_SCAN_CHUNKED) == 0
    case = _case(FP32, L, 128, "gated")
    fig = _worst(case, *_run(gpu, case, "gated", None))
    print(f"scan_fwd gated fp32 L {L}: worst error / bound  out {fig[0]:.3f}  states {fig[1]:.3f}")
    assert max(fig) <= 1.0, fig


def test_tiny_diffma_at_256_tokens_samples_on_the_chunked_scan(gpu, monkeypatch):
    """DiffMa(input_size=32, patch_size=2, hidden_size=64, depth=2) (256 tokens) in eval mode under bf16 autocast: every scan launch
    is one the library gives to the chunk-parallel forward; the output is finite, agrees with the sequential kernel's
    (DIFFMA_SCAN_CHUNKED_LONG off) within rtol 3e-2, atol 5e-2 max|y|, and one hipGraph replay is bit-equal to the eager call."""
    from diffma_amd import _lib, hip_ops
    from diffma_amd.graphed import GraphedDenoiser
    from diffma_amd.model import DiffMa
    from tests.test_model_gpu import _rerandomize

    torch.manual_seed(21)
    net = DiffMa(input_size=32, patch_size=2, hidden_size=64, depth=2)
    _rerandomize(net, 22)
    L, B = 256, 2
    g = torch.Generator().manual_seed(23)
    x, y, y2 = torch.randn(B, 4, 32, 32, generator=g), torch.randn(B, 64, generator=g), torch.randn(B, L, 64, generator=g)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g))
    t = torch.tensor([437, 12])
    net = net.to(gpu).eval()
    x, y, y2, w, t = (v.to(gpu) for v in (x, y, y2, w, t))
    log = []
    real_call, real_call_n = _lib.call, _lib.call_n
    monkeypatch.setattr(_lib, "call", lambda name, a, st: (log.append((name, a)), real_call(name, a, st))[1])
    monkeypatch.setattr(_lib, "call_n", lambda name, arr, st: (log.extend((name, a) for a in arr), real_call_n(name, arr, st))[1])

    def segments():
        seg = [hip_ops.scan_fwd_segment(a.nseq, a.dim, a.seqlen, a.dstate, a.flags) for n, a in log if n == "dm_selective_scan_fwd"]
        assert len(seg) == 4 and all(a.seqlen == L for n, a in log if n == "dm_selective_scan_fwd"), seg       # two mixers x two blocks
        del log[:]
        return seg

    monkeypatch.setattr(hip_ops, "SCAN_CHUNKED_LONG", True)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        eager = net(x, t, y=y, y2=y2, w=w)
        assert all(s > 0 for s in segments())
        monkeypatch.setattr(hip_ops, "SCAN_CHUNKED_LONG", False)
        seq = net(x, t, y=y, y2=y2, w=w)
        assert all(s == 0 for s in segments())
        monkeypatch.setattr(hip_ops, "SCAN_CHUNKED_LONG", True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eager.float()).all()) and float(eager.float().abs().mean()) > 1e-3
    torch.testing.assert_close(eager.float(), seq.float(), rtol=3e-2, atol=5e-2 * float(seq.float().abs().max()))
    gd = GraphedDenoiser(net, x, t, y, y2, w, autocast_dtype=torch.bfloat16, snapshot_weights=False)
    torch.testing.assert_close(gd(x, t, y=y, y2=y2, w=w).clone(), eager, rtol=0, atol=0)
