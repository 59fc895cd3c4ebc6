"""GPU parity of the chunk-parallel backward scan past one segment (csrc/scan_bwd_chunked.h: 196 < L <= 1024, the sequence walked
from its last segment of G tokens to its first with the adjoint carry handed on between them) against fp64 autograd of the oracle,
on inputs where the state remembers (with the plain inputs whatever crosses a segment boundary has decayed to 1e-10 and a wrong
carry is invisible).  The same inputs through the sequential kernel must stay inside the same bounds in the same test.  Checks and
tolerances are those of tests/test_kernels_gpu.py (_scan_bwd_case, _hoisted_scan_case).
"""
import pytest
import torch

from tests.test_kernels_gpu import _hoisted_scan_case, _inputs, _inputs_long_memory, _scan_bwd_case

pytestmark = pytest.mark.gpu

N = 16
NW = 7                         # waves per workgroup = chunks per segment
ONE = 196                      # up to here a launch is one segment (the kernel as it was)
WAVES = 256                    # channel-waves (nseq * ceil(dim / 64)) up to which the library takes the family unforced past 196
                               # tokens: one round of workgroups, profiles/scan_bwd_chunked_long.json (512 up to 196 tokens, as before)
FP32, BF16, FP16 = torch.float32, torch.bfloat16, torch.float16


def _G():
    from diffma_amd import hip_ops

    g = hip_ops.scan_bwd_segment(3, 128, 256, N, 0)
    assert g > 0, "a 3-sequence, 128-channel launch at 256 tokens must take the chunk-parallel backward"
    return g


def _len(spec):
    """A length is a number of tokens, or (g, c, k) = g segments + c wave chunks + k tokens of the geometry the library reports."""
    if isinstance(spec, int):
        return spec
    g, c, k = spec
    return g * _G() + c * (_G() // NW) + k


_LENGTHS = {"G+1": (1, 0, 1), "256": 256, "2G": (2, 0, 0), "2G+1": (2, 0, 1), "2G+LC+3": (2, 1, 3), "1024": 1024}


@pytest.mark.parametrize("dtype,L", [(FP32, k) for k in _LENGTHS] + [(dt, k) for dt in (BF16, FP16) for k in ("G+1", "256", "2G+LC+3", "1024")],
                         ids=lambda v: v if isinstance(v, str) else str(v).replace("torch.", ""))
def test_every_gradient_against_fp64_autograd(gpu, dtype, L):
    """Three directions of one sample through random row tables sharing z and the merged gradient, gated + softplus in the scan: the
    sequential kernel and the chunk-parallel one on the same long-memory inputs, each inside _scan_bwd_case's bounds.  With G = 196:
    G + 1 is the shortest segmented launch (a one-token last segment, six empty waves), 2G ends in a full segment, 2G + 1 in a
    one-token one, 2G + LC + 3 in a ragged chunk whose last sub-chunk is partial (L % 4 = 3).  bf16 and fp16 at 1024 tokens are in
    because the sequential kernel stays inside the bounds there too (both arms measured inside them on one MI355X before the cases
    were added)."""
    from diffma_amd import _lib, hip_ops

    L = _len(_LENGTHS[L])
    assert L > ONE and hip_ops.scan_bwd_segment(3, 128, L, N, _lib.DM_FLAG_SCAN_CHUNKED) == _G()
    for variant in ("sequential", "chunked"):
        _scan_bwd_case(gpu, dtype, 3, L, 128, N, seed=11 * L, indexed=True, Bsz=1, variant=variant, long_memory=True)


@pytest.mark.parametrize("dtype,S,Dm,kw", [
    (FP32, 2, 200, dict()),                                                      # ragged channel block, no row tables
    (FP32, 3, 128, dict(indexed=True, Bsz=1, with_z=False)),                     # no gate
    (FP32, 3, 128, dict(indexed=True, Bsz=1, delta_softplus=False)),             # delta + bias as it is
    (BF16, 3, 128, dict(indexed=True, Bsz=1, bc_fp32=True)),                     # bf16 I/O with fp32 B / C
    (FP32, 3, 128, dict(indexed=True, Bsz=1, a_shared=True, dout_per_seq=True)),  # the Mamba-2 pattern
    (BF16, 3, 128, dict(indexed=True, Bsz=1, a_shared=True, dout_per_seq=True)),
], ids=["dim200", "no-z", "no-softplus", "bf16-fp32bc", "ashared-fp32", "ashared-bf16"])
def test_call_patterns(gpu, dtype, S, Dm, kw):
    _scan_bwd_case(gpu, dtype, S, 256, Dm, N, seed=2560 + Dm, variant="chunked", long_memory=True, **kw)


@pytest.mark.parametrize("dtype", [FP32, BF16, FP16])
def test_hoisted_softplus_launch_of_the_mixer(gpu, dtype):
    """No z, row tables, delta already activated (DM_FLAG_DELTA_ACTIVATED), the pre-gated gradient shared by the directions."""
    _hoisted_scan_case(gpu, dtype, 1, 256, 128, 3, "chunked", seed=2561, long_memory=True)


def _launches(gpu, S, L, Dm, dtype, variants, long_memory=True, seed=5):
    """The backward of one set of inputs (checkpoints from the sequential forward) under each variant: {variant: results}."""
    from diffma_amd import hip_ops

    _, d = (_inputs_long_memory if long_memory else _inputs)(S, L, Dm, N, dtype, seed=seed, dev=gpu)
    ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dtype, gpu).zero_()
    hip_ops.scan_fwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["bias"], True, ckpt=ckpt, variant="sequential")
    dout = torch.randn(S, L, Dm, generator=torch.Generator().manual_seed(seed + 1)).to(dtype).to(gpu)
    got = [(v, hip_ops.scan_bwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["bias"], dout, ckpt, True, variant=v))
           for v in variants]
    torch.cuda.synchronize()
    return got


def _same_bits(a, b):
    return all((x is None and y is None) or torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def test_library_choice_is_the_chunked_kernel_and_is_deterministic(gpu, monkeypatch):
    """variant=None (the library's own choice) is bit-equal to variant="chunked" at 256 tokens, run twice; the sequential kernel
    gives other bits, so the comparison can tell them apart; with SCAN_BWD_CHUNKED_LONG off the library's choice is the sequential
    kernel."""
    from diffma_amd import _lib, hip_ops

    assert _lib.load().dm_scan_bwd_launch_group_channels(3, 128, 256, N, 0) == 64
    monkeypatch.setattr(hip_ops, "SCAN_BWD_CHUNKED_LONG", True)
    r = [res for _, res in _launches(gpu, 3, 256, 128, FP32, (None, "chunked", "chunked", "sequential"))]
    assert _same_bits(r[0], r[1]) and _same_bits(r[1], r[2])
    assert not _same_bits(r[0], r[3])
    assert not torch.equal(r[0][0], r[3][0]) or not torch.equal(r[0][5], r[3][5])         # du or dA: other bits
    monkeypatch.setattr(hip_ops, "SCAN_BWD_CHUNKED_LONG", False)
    off = [res for _, res in _launches(gpu, 3, 256, 128, FP32, (None,))]
    assert _same_bits(off[0], r[3])


@pytest.mark.parametrize("S,chunked", [(WAVES // 16, True), (WAVES // 16 + 1, False)])
def test_routing_threshold(gpu, S, chunked):
    """One launch on each side of the channel-wave threshold at L = 197, 1024 channels (16 channel-waves per sequence): the
    library's choice leaves the bits of the chunk-parallel kernel up to it and those of the sequential one past it."""
    from diffma_amd import hip_ops

    assert (hip_ops.scan_bwd_segment(S, 1024, 197, N, 0) > 0) == chunked
    got = dict(_launches(gpu, S, 197, 1024, BF16, (None, "chunked", "sequential"), long_memory=False, seed=S))
    assert not _same_bits(got["chunked"], got["sequential"])
    assert _same_bits(got[None], got["chunked" if chunked else "sequential"])


def test_pair_is_one_launch_and_bit_equal_to_two(gpu, monkeypatch):
    """Two congruent structs at L 256 through dm_selective_scan_bwd_n, as hip_ops.both issues them: one call, the bits of two."""
    from diffma_amd import _lib, hip_ops

    S, L, Dm = 3, 256, 128
    _, d = _inputs_long_memory(S, L, Dm, N, BF16, seed=77, dev=gpu, with_z=False)
    g = torch.Generator().manual_seed(78)
    idx = torch.stack([torch.randperm(L, generator=g) for _ in range(3)]).int().to(gpu)
    act = torch.nn.functional.softplus(d["delta"].float() + d["bias"]).to(BF16)
    dout = torch.randn(1, L, Dm, generator=g).to(BF16).to(gpu)
    first = dict(u=d["u"], act=act, A=d["A"], B=d["B"], C=d["C"], D=d["D"], bias=d["bias"], dout=dout)
    ops = [first, dict(first, u=first["u"].flip(0).contiguous(), A=first["A"] * 0.5, B=first["C"], C=first["B"])]     # congruent, other data
    kw = dict(z_row_index=idx, out_row_index=idx, batch_per_dir=1, delta_activated=True)
    for o in ops:
        o["ckpt"] = hip_ops.alloc_scan_ckpt(S, L, N, Dm, BF16, gpu).zero_()
        hip_ops.scan_fwd(o["u"], o["act"], o["A"], o["B"], o["C"], o["D"], None, o["bias"], True, ckpt=o["ckpt"], variant="sequential", **kw)
    launch = lambda o: hip_ops.scan_bwd(o["u"], o["act"], o["A"], o["B"], o["C"], o["D"], None, o["bias"], o["dout"], o["ckpt"], True, **kw)
    single = [launch(o) for o in ops]
    calls = []
    real, real_n = _lib.call, _lib.call_n
    monkeypatch.setattr(_lib, "call", lambda name, a, st: (calls.append((name, 1)), real(name, a, st))[1])
    monkeypatch.setattr(_lib, "call_n", lambda name, arr, st: (calls.append((name, len(arr))), real_n(name, arr, st))[1])
    pair = hip_ops.both(lambda i: launch(ops[i]))
    torch.cuda.synchronize()
    assert [c for c in calls if c[0].startswith("dm_selective_scan")] == [("dm_selective_scan_bwd", 2)], calls
    assert not _same_bits(single[0], single[1])
    for a, b in zip(single, pair):
        assert _same_bits(a, b)


def test_1025_tokens_stay_on_the_sequential_kernel(gpu):
    from diffma_amd import _lib, hip_ops

    lib = _lib.load()
    for flags in (0, _lib.DM_FLAG_SCAN_CHUNKED):
        assert hip_ops.scan_bwd_segment(3, 128, 1025, N, flags) == 0 and lib.dm_scan_bwd_launch_group_channels(3, 128, 1025, N, flags) == 256
    _scan_bwd_case(gpu, FP32, 3, 1025, 128, N, seed=1025, indexed=True, Bsz=1, variant=None, long_memory=True)


@pytest.mark.parametrize("hidden", [64, 128])
def test_tiny_diffma_at_256_tokens_trains_on_the_chunked_backward(gpu, monkeypatch, hidden):
    """DiffMa(input_size=32, patch_size=2, hidden_size=64, depth=2) (256 tokens), batch 2, one forward + backward under bf16 autocast:
    every backward scan is one the library gives to the chunk-parallel kernel, the parameter gradients are finite and agree with
    the sequential kernel's (DIFFMA_SCAN_BWD_CHUNKED_LONG off) within rtol 3e-2, atol 5e-2 max|grad| per tensor.  The two mixers of
    a block leave as one launch wherever the model takes its pair path at all: that path needs the fused dt_proj + softplus, which
    is built for dt_rank + 32 a multiple of 8, and the mixers' dt_rank is hidden_size / 16 -- 4 at hidden_size 64, where the four
    launches leave one by one whatever the scan does, 8 at hidden_size 128, where they must pair."""
    from diffma_amd import _lib, hip_ops
    from diffma_amd.model import DiffMa
    from diffma_amd.selective_scan_interface import spiral_ssm_pair_supported
    from tests.test_model_gpu import _rerandomize

    torch.manual_seed(21)
    net = DiffMa(input_size=32, patch_size=2, hidden_size=hidden, depth=2)
    _rerandomize(net, 22)
    L, B = 256, 2
    g = torch.Generator().manual_seed(23)
    x, y, y2 = torch.randn(B, 4, 32, 32, generator=g), torch.randn(B, hidden, generator=g), torch.randn(B, L, hidden, generator=g)
    w = torch.sigmoid(torch.randn(B, L, 1, generator=g))
    t = torch.tensor([437, 12])
    net = net.to(gpu).train()
    blk = net.blocks[0]
    paired = spiral_ssm_pair_supported(B, L, torch.bfloat16, blk.mamba1, blk.mamba2)
    assert paired == (hidden == 128)
    x, y, y2, w, t = (v.to(gpu) for v in (x, y, y2, w, t))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        shape = net(x, t, y=y, y2=y2, w=w).shape
    gout = torch.randn(shape, generator=g).to(gpu)
    log, pairs = [], []
    real_call, real_call_n = _lib.call, _lib.call_n
    monkeypatch.setattr(_lib, "call", lambda name, a, st: (log.append((name, a)), real_call(name, a, st))[1])
    monkeypatch.setattr(_lib, "call_n", lambda name, arr, st: (log.extend((name, a) for a in arr), pairs.append((name, len(arr))),
                                                               real_call_n(name, arr, st))[2])

    def step(on):
        monkeypatch.setattr(hip_ops, "SCAN_BWD_CHUNKED_LONG", on)
        del log[:], pairs[:]
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(x, t, y=y, y2=y2, w=w)
        (out.float() * gout).sum().backward()
        torch.cuda.synchronize()
        structs = [a for n, a in log if n == "dm_selective_scan_bwd"]
        assert len(structs) == 4 and all(a.seqlen == L for a in structs)                     # two mixers x two blocks
        seg = [hip_ops.scan_bwd_segment(a.nseq, a.dim, a.seqlen, a.dstate, a.flags) for a in structs]
        return {n: p.grad.detach().float().clone() for n, p in net.named_parameters() if p.grad is not None}, seg, list(pairs)

    grads, seg, prs = step(True)
    assert all(s > 0 for s in seg), seg
    assert [p for p in prs if p[0] == "dm_selective_scan_bwd"] == ([("dm_selective_scan_bwd", 2)] * 2 if paired else []), prs
    assert grads and all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert sum(float(v.abs().sum()) for v in grads.values()) > 0
    ref, seg_off, _ = step(False)
    assert all(s == 0 for s in seg_off), seg_off
    assert grads.keys() == ref.keys()
    for n in ref:
        torch.testing.assert_close(grads[n], ref[n], rtol=3e-2, atol=5e-2 * float(ref[n].abs().max()), msg=lambda m, n=n: f"{n}: {m}")
