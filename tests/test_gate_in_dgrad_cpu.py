"""dm_gemm_large with its gated epilogue (gate_z set; csrc/gemm_large.hip): the out_proj input gradient with the hoisted gate's backward in its epilogue -- the
parts that need no GPU.  tests/test_gate_in_dgrad_gpu.py imports the builders and the shape table from here.

What the entry point promises (include/diffma_hip.h): with dy = A B^T rounded to the I/O dtype, g = dy silu(z) and dz = dy pre silu'(z)
are what dm_gemm_large followed by dm_gate_bwd write, bit for bit; dy is not stored.  The GPU file compares against exactly that pair.
Where a last place could differ (1 + z (1 - sg) is open to contraction into an FMA, per instantiation: tests/test_mixer_passes_gpu.py)
the difference is held to the dm_gate_bwd bounds of tests/test_mixer_passes_cpu.py against fp64 -- no tolerance of this file's own.

Here: the header's view of the new fields and symbols, the row split between the persistent kernel and the small-launch kernel
(dm_gemm_large_tail_rows), the support query, every refusal (they return before anything touches the device, so fake addresses do), and
the routing predicate on tensors that cannot take the path.
"""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

from tests.test_mixer_passes_cpu import BF16, DM_ERR_ARG, DM_ERR_DTYPE, DM_ERR_LAYOUT, F16, F32, z_values

Q = 1024                      # d_inner of the smallest block that takes K12
ROUND = 256 // (Q // 256) * 256               # rows of ONE round of 256 x 256 tiles on 256 CUs: 256 tiles / 4 column tiles = 64 row blocks
# (name, P, Kc): one whole round; the same plus 300 rows (the remainder goes to dm_gemm + dm_gate_bwd: the seam); two K groups; a
# remainder of half a round or more, which stays in the persistent kernel and ends in a partial row block; the contraction the issue
# names that K12 does not take (Kc % 512 != 0): both entry points refuse it.
SHAPES = [("round", ROUND, 512), ("round+300", ROUND + 300, 512), ("round_k1024", ROUND, 1024), ("partial_block", 97 * 256 - 100, 512),
          ("round_k64", ROUND, 64)]
TAIL = {"round": 0, "round+300": 300, "round_k1024": 0, "partial_block": 0, "round_k64": 0}


def gated_case(dt, P, Kc, seed=0):
    """d(out) [P, Kc] and the transposed weight [Q, Kc] (dy = A B^T of order 1), z over its value classes, pre at 1e-2 .. 1e2."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(P, Kc, generator=g).to(dt)
    b = (torch.randn(Q, Kc, generator=g) * Kc ** -0.5).to(dt)
    z = z_values((1, P, Q), g)[0].to(dt)
    pre = (torch.randn(P, Q, generator=g) * 10.0 ** (4 * torch.rand(P, Q, generator=g) - 2)).to(dt)
    return NS(dt=dt, P=P, Q=Q, Kc=Kc, a=a, b=b, z=z, pre=pre)


def _lib():
    from diffma_amd import _lib as L

    return L


def test_round_is_64_row_blocks():
    assert ROUND == 16384


def gated_args(P, Qq, Kc, code, a, b, z, pre, g, dz, dy_tail=0, lda=None, ldb=None, ldz=None, ldp=None, ldg=None, lddz=None, ld_tail=None):
    """dm_gemm_args of a gated dm_gemm_large call: addresses as integers; c / ldc carry the remainder's dy slice."""
    s = _lib().dm_gemm_args()
    s.P, s.Q, s.Kc, s.ab_dtype, s.c_dtype, s.a_kmajor, s.b_kmajor, s.accumulate = P, Qq, Kc, code, code, 1, 1, 0
    s.a, s.b, s.c, s.gate_z, s.gate_pre, s.gate_g, s.gate_dz = a, b, dy_tail, z, pre, g, dz
    s.lda, s.ldb, s.ldc = Kc if lda is None else lda, Kc if ldb is None else ldb, Qq if ld_tail is None else ld_tail
    s.gate_ldz, s.gate_ldp = 2 * Qq if ldz is None else ldz, Qq if ldp is None else ldp
    s.gate_ldg, s.gate_lddz = Qq if ldg is None else ldg, 2 * Qq if lddz is None else lddz
    return s


def test_header_declares_the_gated_fields():
    L = _lib()
    assert L.CONSTANTS["DM_ABI_VERSION"] >= 33
    fields = [f for f, _ in L.STRUCT_FIELDS["dm_gemm_args"]]
    assert fields[-8:] == ["gate_z", "gate_pre", "gate_g", "gate_dz", "gate_ldz", "gate_ldp", "gate_ldg", "gate_lddz"]
    assert "dm_gemm_gated_args" not in L.STRUCT_FIELDS and "dm_gemm_large_gated" not in L.EXPORTED_SYMBOLS       # one form only
    for name in ("dm_gemm_large_gated_supported", "dm_gemm_large_tail_rows"):
        assert name in L.EXPORTED_SYMBOLS
    assert L.load().dm_abi_version() == L.CONSTANTS["DM_ABI_VERSION"]


def test_tail_rows_follow_the_whole_round_rule():
    """Whole rounds of 256 tiles go to the persistent kernel; what is left goes to dm_gemm unless it is half a round or more."""
    lib = _lib().load()
    for name, P, _ in SHAPES:
        assert lib.dm_gemm_large_tail_rows(P, Q) == TAIL[name], name
    assert lib.dm_gemm_large_tail_rows(100352, 1024) == 2048          # the bench batch: 392 row blocks, 384 in six rounds
    assert lib.dm_gemm_large_tail_rows(100352, 2048) == 2048          # eight column tiles: 64 tiles are left, a quarter round
    assert lib.dm_gemm_large_tail_rows(ROUND + 31 * 256, 1024) == 31 * 256      # 124 tiles: below half a round
    assert lib.dm_gemm_large_tail_rows(ROUND + 32 * 256, 1024) == 0             # 128 tiles: half a round stays
    assert lib.dm_gemm_large_tail_rows(0, 1024) == 0 and lib.dm_gemm_large_tail_rows(4096, 1000) == 0


def test_supported_matches_dm_gemm_large():
    lib = _lib().load()
    for P, Qq, Kc, code, want in [(ROUND, Q, 512, 1, 1), (ROUND, Q, 512, 2, 1), (ROUND, Q, 1024, 1, 1), (ROUND, Q, 64, 1, 0),
                                  (ROUND, Q, 512, 0, 0), (ROUND, 1000, 512, 1, 0), (ROUND, 1032, 512, 1, 0), (2047, Q, 512, 1, 0),
                                  (ROUND, Q, 768, 1, 0)]:
        assert lib.dm_gemm_large_gated_supported(P, Qq, Kc, code) == want, (P, Qq, Kc, code)
        assert lib.dm_gemm_large_supported(P, Qq, Kc, 1, 1, code, code) == want


def _fake_args(P=ROUND, Qq=Q, Kc=512, code=1, **kw):
    """A struct whose addresses are aligned numbers, never dereferenced: every case below is refused by the host checks."""
    names = ("a", "b", "z", "pre", "g", "dz", "dy_tail")
    ptrs = {n: 0x10000 * (i + 1) for i, n in enumerate(names)}
    raw = {k: kw.pop(k) for k in ("c_dtype", "accumulate", "a_kmajor") if k in kw}
    ptrs.update(kw)
    s = gated_args(P, Qq, Kc, code, **ptrs)
    for k, v in raw.items():
        setattr(s, k, v)
    return s


REFUSALS = [(dict(code=0), DM_ERR_DTYPE), (dict(code=5), DM_ERR_DTYPE), (dict(Kc=64), DM_ERR_ARG), (dict(Kc=768), DM_ERR_ARG),
            (dict(Qq=1000), DM_ERR_ARG), (dict(Qq=1032), DM_ERR_ARG), (dict(P=2047), DM_ERR_ARG),
            (dict(a=0), DM_ERR_ARG), (dict(b=0), DM_ERR_ARG), (dict(pre=0), DM_ERR_ARG), (dict(g=0), DM_ERR_ARG),
            (dict(dz=0), DM_ERR_ARG), (dict(P=ROUND + 300, dy_tail=0), DM_ERR_ARG),
            (dict(a=0x10002), DM_ERR_LAYOUT), (dict(b=0x20008), DM_ERR_LAYOUT), (dict(z=0x30002), DM_ERR_LAYOUT),
            (dict(pre=0x40004), DM_ERR_LAYOUT), (dict(g=0x50008), DM_ERR_LAYOUT), (dict(dz=0x6000e), DM_ERR_LAYOUT),
            (dict(P=ROUND + 300, dy_tail=0x70002), DM_ERR_LAYOUT), (dict(P=ROUND + 300, ld_tail=Q - 8), DM_ERR_LAYOUT),
            (dict(lda=516), DM_ERR_LAYOUT), (dict(ldz=2 * Q + 4, lddz=2 * Q + 4), DM_ERR_LAYOUT), (dict(ldp=Q - 8, ldg=Q - 8), DM_ERR_LAYOUT),
            (dict(lddz=2 * Q + 8), DM_ERR_LAYOUT), (dict(ldg=Q + 8), DM_ERR_LAYOUT),
            (dict(P=600000, ldz=2 * Q, lddz=2 * Q), DM_ERR_LAYOUT),
            (dict(c_dtype=0), DM_ERR_ARG), (dict(accumulate=1), DM_ERR_ARG), (dict(a_kmajor=0), DM_ERR_ARG)]


@pytest.mark.parametrize("kw,want", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_refusals_return_before_any_launch(kw, want):
    """fp32 and unknown dtypes; a contraction or a width K12 does not take (1000 is no multiple of the 8-element row piece either);
    null pointers (a NULL gate_z is the plain call, not a refusal); a remainder without its dy slice; every pointer off its 16-byte boundary; strides that are no multiple of 8, do
    not cover a row, or differ between z and dz / pre and g; a tensor past 2 GB; an fp32 C, accumulation, a row-major operand."""
    lib = _lib().load()
    assert int(lib.dm_gemm_large(ctypes.byref(_fake_args(**kw)), None)) == want, lib.dm_last_error().decode()


def test_dm_gemm_refuses_the_gate_fields():
    lib = _lib().load()
    assert int(lib.dm_gemm(ctypes.byref(_fake_args(P=256)), None)) == DM_ERR_ARG
    assert b"gate_z" in lib.dm_last_error()


def test_routing_rule_condition_by_condition(monkeypatch):
    """The bench mixer (512 x 196 tokens, d_model 512, d_inner 1024, bf16) takes the path; every single condition of the issue turned
    the other way does not: each switch, fp32, a host tensor, an autocast dtype that differs, no backward, a strided xz, fewer rows
    than LARGE_MIN_ROWS, an out_proj narrower than LARGE_MIN_COLS, a width K12 does not take, a contraction it does not take, an xz
    that is not [.., 2 d_inner]."""
    from diffma_amd import hip_ops, projections as proj, selective_scan_interface as ssi

    monkeypatch.setattr(hip_ops, "GATE_IN_DGRAD", True)
    base = dict(on_gpu=True, dtype=BF16, autocast_dtype=BF16, contiguous=True, wants_grad=True, xz_shape=(512, 196, 2048), w_shape=(512, 1024))
    rule = lambda **kw: ssi._gate_in_dgrad_rule(**{**base, **kw})
    assert rule() and rule(dtype=F16, autocast_dtype=F16) and rule(autocast_dtype=None)
    assert rule(xz_shape=(64, 196, 2048))                              # 12 544 rows: the smallest batch of 196 tokens above LARGE_MIN_ROWS
    for kw in (dict(on_gpu=False), dict(dtype=F32, autocast_dtype=None), dict(autocast_dtype=F16), dict(wants_grad=False), dict(contiguous=False),
               dict(xz_shape=(62, 196, 2048)), dict(xz_shape=(512, 196, 1024), w_shape=(512, 512)),
               dict(xz_shape=(512, 196, 2000), w_shape=(512, 1000)), dict(w_shape=(576, 1024)), dict(xz_shape=(512, 196, 4096)),
               dict(xz_shape=(512 * 196, 2048))):
        assert not rule(**kw), kw
    for mod, name in ((hip_ops, "GATE_IN_DGRAD"), (ssi, "HOIST_GATE"), (proj, "LARGE_DGRAD_NT"), (hip_ops, "GEMM_LARGE")):
        with monkeypatch.context() as mp:
            mp.setattr(mod, name, False)
            assert not rule(), name
    assert proj.LARGE_MIN_ROWS > proj.PAIR_OWN_MAX_ROWS                   # the small-launch kernel's range lies below the path
    xz = torch.zeros(64, 196, 2048, dtype=BF16, requires_grad=True)    # the tensor form: a host tensor never takes it
    assert not ssi.gate_in_dgrad_wanted(xz, torch.zeros(512, 1024))
