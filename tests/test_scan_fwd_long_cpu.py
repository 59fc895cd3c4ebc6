"""The chunk-parallel forward scan past one segment (csrc/scan_fwd_chunked.h, 196 < L <= 1024), the parts that need no GPU: the
launch query dm_scan_fwd_launch_segment, the DIFFMA_SCAN_CHUNKED_LONG switch on the flag word, and an fp64 restatement of the
segmented two-pass scheme against the plain recurrence.
"""
import math

import pytest
import torch

G1 = 196                       # one segment: 14 waves x 14 steps, today's launches
NW, LC = 14, 10                # past 196 tokens: 14 waves x 10 steps per segment
G = NW * LC


def test_symbol_and_abi():
    from diffma_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "dm_scan_fwd_launch_segment") and "dm_scan_fwd_launch_segment" in _lib.ARGTYPES
    assert lib.dm_abi_version() >= 35 and _lib.CONSTANTS["DM_ABI_VERSION"] >= 35


@pytest.mark.parametrize("S,Dm,L,N,flag,want", [
    (3, 2048, 256, 16, None, G), (24, 1024, 1024, 16, None, G), (6, 128, 197, 16, None, G),
    (3, 2048, 1025, 16, None, 0),                       # past the longest sequence the family serves
    (3, 2048, 1025, 16, "DM_FLAG_SCAN_CHUNKED", 0),     # ... which forcing does not change
    (3, 2048, 256, 16, "DM_FLAG_SCAN_SEQUENTIAL", 0),
    (3, 2048, 256, 32, None, 0),                        # d_state 16 only
    (32, 1024, 256, 16, None, G), (33, 1024, 256, 16, None, 0), (8, 2048, 1024, 16, None, G),       # 512 channel-waves and one more
    (768, 1024, 256, 16, None, 0),                      # 12 288 channel-waves: far over the size threshold
    (768, 1024, 256, 16, "DM_FLAG_SCAN_CHUNKED", G),    # ... and forced
    (6, 128, 100, 16, None, G1), (6, 128, 196, 16, None, G1),
    (6, 128, 56, 16, None, 0),                          # too short to cut
])
def test_query_table(S, Dm, L, N, flag, want):
    from diffma_amd import _lib, hip_ops

    flags = 0 if flag is None else getattr(_lib, flag)
    assert _lib.load().dm_scan_fwd_launch_segment(S, Dm, L, N, flags) == want
    assert hip_ops.scan_fwd_segment(S, Dm, L, N, flags) == want
    assert hip_ops.SCAN_CHUNKED_SEGMENT == G1


@pytest.mark.parametrize("on", [True, False])
def test_switch_sets_the_sequential_flag_past_one_segment(monkeypatch, on):
    """The flag word of the launch itself (no device: the launch is captured, the tensors live on the host)."""
    from diffma_amd import _lib, hip_ops

    monkeypatch.setattr(hip_ops, "SCAN_CHUNKED_LONG", on)
    got = []
    monkeypatch.setattr(hip_ops, "_launch", lambda name, a, *rest, **kw: got.append((name, a.seqlen, a.flags)))
    S, Dm, N = 2, 64, 16
    for L in (256, 196):
        for variant in (None, "chunked", "sequential"):
            u = torch.zeros(S, L, Dm)
            hip_ops._scan_fwd_launch(u, u, torch.zeros(Dm, N), torch.zeros(S, L, N), torch.zeros(S, L, N), None, None, None, True, None, None,
                                     0, torch.empty_like(u), None, hip_ops.SCAN_CKPT_EVERY, None, 1, False, variant, False)
    seq, chk = _lib.DM_FLAG_SCAN_SEQUENTIAL, _lib.DM_FLAG_SCAN_CHUNKED
    fam = [(L, f & (seq | chk)) for _, L, f in got]
    assert all(n == "dm_selective_scan_fwd" for n, _, _ in got) and all(f & _lib.DM_FLAG_DELTA_SOFTPLUS for _, _, f in got)
    assert fam == [(256, 0 if on else seq), (256, chk), (256, seq), (196, 0), (196, chk), (196, seq)]


def _long_memory(L, Dm, N, seed):
    """fp64 inputs where the state remembers (tests/test_kernels_gpu.py _inputs_long_memory): A = -(n + 1) c_d, c_d in [0.01, 1],
    dt log-uniform per channel in [1e-3, 1e-1] times exp(0.3 randn)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = torch.exp(torch.rand(Dm, generator=g, dtype=torch.float64) * math.log(100.0)) * 0.01
    A = -(torch.arange(N, dtype=torch.float64) + 1.0)[None, :] * c[:, None]
    level = torch.exp(torch.rand(Dm, generator=g, dtype=torch.float64) * math.log(100.0)) * 1e-3
    return level * torch.exp(0.3 * rnd(L, Dm)), rnd(L, Dm), rnd(L, N), A


def _step(h, dt, u, B, A, l):
    return torch.exp(dt[l][:, None] * A) * h + (dt[l] * u[l])[:, None] * B[l][None, :]


def _segmented(dt, u, B, A):
    """The kernel's scheme: per segment of G tokens, chunk c = LC steps (ragged or empty at the end); every chunk's end state from
    zero and its decay P = exp(A sum dt); the state entering chunk c is the fold x <- P_j x + h_j over j < c started from the
    state entering the segment; the fold continued over all NW chunks is the state entering the next segment."""
    L, z = dt.shape[0], torch.zeros_like(A)
    H, states = z, []
    for g0 in range(0, L, G):
        pub = []
        for c in range(NW):
            lo = min(g0 + c * LC, L)
            hi = min(lo + LC, L)
            h = z
            for l in range(lo, hi):
                h = _step(h, dt, u, B, A, l)
            pub.append((torch.exp(A * dt[lo:hi].sum(0)[:, None]), h, lo, hi))
        x = H
        for P, hc, lo, hi in pub:
            h = x                                        # pass 2 from the folded entry state
            for l in range(lo, hi):
                h = _step(h, dt, u, B, A, l)
                states.append(h)
            x = P * x + hc
        H = x
    return torch.stack(states), H


@pytest.mark.parametrize("L", [G + 1, 2 * G, 2 * G + 1, 2 * G + LC + 3])
def test_segmented_two_pass_scheme_is_the_recurrence(L):
    Dm, N = 8, 16
    dt, u, B, A = _long_memory(L, Dm, N, seed=L)
    h, ref = torch.zeros_like(A), []
    for l in range(L):
        h = _step(h, dt, u, B, A, l)
        ref.append(h)
    ref = torch.stack(ref)
    got, carry = _segmented(dt, u, B, A)
    scale = float(ref.abs().max())
    assert float((ref[G] - _step(torch.zeros_like(A), dt, u, B, A, G)).abs().max()) > 0.1 * scale       # a dropped carry would show
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * scale
    assert float((carry - ref[-1]).abs().max()) <= 1e-12 * scale          # the fold over every chunk = the state after the last step
