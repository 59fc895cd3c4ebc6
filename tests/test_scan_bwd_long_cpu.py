"""The chunk-parallel backward scan past one segment (csrc/scan_bwd_chunked.h, 196 < L <= 1024), the parts that need no GPU: the
launch queries dm_scan_bwd_launch_segment / dm_scan_bwd_launch_group_channels, the DIFFMA_SCAN_BWD_CHUNKED_LONG switch on the flag
word, and an fp64 restatement of the reverse segmented two-pass scheme against the plain adjoint recursion.
"""
import pytest
import torch

from tests.test_scan_fwd_long_cpu import _long_memory

NW = 7                         # waves per workgroup = chunks per segment
G1, G1S = 196, 56              # today's one-segment launches: 7 waves x 28 steps, 7 x 8 for the short ones
WAVES = 256                    # channel-waves (nseq * ceil(dim / 64)) up to which the library takes the family unforced past 196
                               # tokens: one round of workgroups, profiles/scan_bwd_chunked_long.json (512 up to 196 tokens, as before)


def _G():
    from diffma_amd import hip_ops

    g = hip_ops.scan_bwd_segment(3, 128, 256, 16, 0)
    assert g > 0 and g % NW == 0 and (g // NW) % hip_ops.SCAN_CKPT_EVERY == 0, g
    return g


def test_symbol_and_abi():
    from diffma_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "dm_scan_bwd_launch_segment") and "dm_scan_bwd_launch_segment" in _lib.ARGTYPES
    assert lib.dm_abi_version() >= 36 and _lib.CONSTANTS["DM_ABI_VERSION"] >= 36


@pytest.mark.parametrize("S,Dm,L,N,flag,want", [
    (6, 128, 197, 16, None, "G"), (6, 128, 256, 16, None, "G"), (6, 128, 1024, 16, None, "G"),
    (6, 128, 1025, 16, None, 0),                        # past the longest sequence the family serves
    (6, 128, 1025, 16, "DM_FLAG_SCAN_CHUNKED", 0),      # ... which forcing does not change
    (6, 128, 256, 16, "DM_FLAG_SCAN_SEQUENTIAL", 0),
    (6, 128, 256, 32, None, 0),                         # d_state 16 only
    (WAVES // 16, 1024, 256, 16, None, "G"), (WAVES // 16 + 1, 1024, 256, 16, None, 0),     # the size threshold and one past it
    (WAVES // 32, 2048, 1024, 16, None, "G"), (WAVES // 32 + 1, 2048, 1024, 16, None, 0),
    (768, 1024, 256, 16, None, 0),                      # 12 288 channel-waves: far over the size threshold
    (768, 1024, 256, 16, "DM_FLAG_SCAN_CHUNKED", "G"),  # ... and forced
    (6, 128, 196, 16, None, G1), (6, 128, 100, 16, None, G1), (6, 128, 60, 16, None, G1),           # today's answers
    (6, 128, 20, 16, None, G1S), (6, 128, 16, 16, None, 0),
    (768, 1024, 196, 16, None, 0), (768, 1024, 196, 16, "DM_FLAG_SCAN_CHUNKED", G1),
])
def test_query_table(S, Dm, L, N, flag, want):
    """The segment query, and the partial-row query that must follow the same rule: 64 channels per dB/dC row exactly where the
    family is taken, the sequential kernel's 256 (d_state 16; 128 at d_state 32) elsewhere."""
    from diffma_amd import _lib, hip_ops

    lib = _lib.load()
    flags = 0 if flag is None else getattr(_lib, flag)
    want = _G() if want == "G" else want
    assert lib.dm_scan_bwd_launch_segment(S, Dm, L, N, flags) == want
    assert hip_ops.scan_bwd_segment(S, Dm, L, N, flags) == want
    assert lib.dm_scan_bwd_launch_group_channels(S, Dm, L, N, flags) == (64 if want else lib.dm_scan_bwd_group_channels(N))
    assert lib.dm_scan_bwd_group_channels(16) == 256


def test_partial_shape_follows_the_query():
    from diffma_amd import _lib, hip_ops

    assert hip_ops.scan_bwd_partial_shape(3, 256, 200, 16) == (3, 256, 4, 32)                  # ceil(200 / 64) rows per step
    assert hip_ops.scan_bwd_partial_shape(3, 256, 200, 16, _lib.DM_FLAG_SCAN_SEQUENTIAL) == (3, 256, 1, 32)
    assert hip_ops.scan_bwd_partial_shape(3, 1025, 200, 16, _lib.DM_FLAG_SCAN_CHUNKED) == (3, 1025, 1, 32)


@pytest.mark.parametrize("on", [True, False])
def test_switch_sets_the_sequential_flag_past_one_segment(monkeypatch, on):
    """The flag word of the backward launch itself and the partial rows sized for it (no device: the launches are captured, the
    tensors live on the host)."""
    from diffma_amd import _lib, hip_ops

    monkeypatch.setattr(hip_ops, "SCAN_BWD_CHUNKED_LONG", on)
    monkeypatch.setattr(hip_ops, "_require_gpu", lambda *ts: None)
    got = []
    monkeypatch.setattr(hip_ops, "_launch", lambda name, a, *rest, **kw: got.append((name, a, rest[0])))
    S, Dm, N = 2, 128, 16
    shapes = []
    for L in (256, 196):
        for variant in (None, "chunked", "sequential"):
            u = torch.zeros(S, L, Dm)
            bc = torch.zeros(S, L, N)
            ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, u.dtype, "cpu")
            res = hip_ops.scan_bwd(u, u, torch.zeros(Dm, N), bc, bc, None, None, None, u, ckpt, True, variant=variant)
            shapes.append(tuple(res[3].shape))
    seq, chk = _lib.DM_FLAG_SCAN_SEQUENTIAL, _lib.DM_FLAG_SCAN_CHUNKED
    bwd = [(a.seqlen, a.flags) for n, a, _ in got if n == "dm_selective_scan_bwd"]
    assert len(bwd) == 6 and all(f & _lib.DM_FLAG_DELTA_SOFTPLUS for _, f in bwd)
    assert [(L, f & (seq | chk)) for L, f in bwd] == [(256, 0 if on else seq), (256, chk), (256, seq), (196, 0), (196, chk), (196, seq)]
    # the partial rows handed to dm_sum_partials were sized AFTER the flag was set: at 128 channels two rows per step where the
    # family is taken (one per 64 channels), one for the sequential kernel
    assert [a.nw for n, a, _ in got if n == "dm_sum_partials"] == [1 if f & seq else 2 for _, f in bwd]
    assert shapes == [(S, L, N) for L in (256, 196) for _ in range(3)]


def _adjoint(dt, gy, C, A):
    """G_l = C_l gy_l + carry,  carry <- exp(dt_l A) G_l,  l = L-1 .. 0."""
    L = dt.shape[0]
    carry, out = torch.zeros_like(A), [None] * L
    for l in range(L - 1, -1, -1):
        out[l] = gy[l][:, None] * C[l][None, :] + carry
        carry = torch.exp(dt[l][:, None] * A) * out[l]
    return torch.stack(out)


def _segmented(dt, gy, C, A, G):
    """The kernel's scheme: segments of G tokens aligned at token 0, walked from the last to the first; chunk c of a segment is
    LC = G / NW steps (ragged or empty past L).  Every chunk publishes its left-going carry from zero c_loc and its decay
    Q = exp(A sum dt); the carry entering chunk c from the right is the fold X <- c_loc(j) + Q(j) X over j = NW-1 .. c+1 started
    from the carry entering the segment; the fold continued over chunk 0 is the carry entering the next segment to the left."""
    L, z = dt.shape[0], torch.zeros_like(A)
    LC = G // NW
    out = [None] * L
    X_seg = z
    for g in range((L + G - 1) // G - 1, -1, -1):
        pub = []
        for c in range(NW):
            lo = min(g * G + c * LC, L)
            hi = min(lo + LC, L)
            carry = z
            for l in range(hi - 1, lo - 1, -1):
                carry = torch.exp(dt[l][:, None] * A) * (gy[l][:, None] * C[l][None, :] + carry)
            pub.append((carry, torch.exp(A * dt[lo:hi].sum(0)[:, None]), lo, hi))
        X = X_seg
        for c in range(NW - 1, -1, -1):
            c_loc, Q, lo, hi = pub[c]
            carry = X                                    # pass 2 from the folded carry
            for l in range(hi - 1, lo - 1, -1):
                out[l] = gy[l][:, None] * C[l][None, :] + carry
                carry = torch.exp(dt[l][:, None] * A) * out[l]
            X = c_loc + Q * X
        X_seg = X
    return torch.stack(out), X_seg


@pytest.mark.parametrize("spec", ["G+1", "256", "2G", "2G+1", "2G+LC+3", "1024"])
def test_reverse_segmented_scheme_is_the_adjoint_recursion(spec):
    G = _G()
    LC = G // NW
    L = {"G+1": G + 1, "256": 256, "2G": 2 * G, "2G+1": 2 * G + 1, "2G+LC+3": 2 * G + LC + 3, "1024": 1024}[spec]
    Dm, N = 8, 16
    dt, gy, C, A = _long_memory(L, Dm, N, seed=L)
    ref = _adjoint(dt, gy, C, A)
    got, left = _segmented(dt, gy, C, A, G)
    scale = float(ref.abs().max())
    worst = float((got - ref).abs().max())
    dropped = float((torch.exp(dt[G][:, None] * A) * ref[G]).abs().max())      # what G_{G-1} loses if the carry at token G is dropped
    print(f"L {L} (G {G}, LC {LC}): scheme - recursion {worst / scale:.2e} x max|G|, dropped carry {dropped / scale:.3f} x max|G|")
    assert got.shape == ref.shape and worst <= 1e-12 * scale
    assert float((left - torch.exp(dt[0][:, None] * A) * ref[0]).abs().max()) <= 1e-12 * scale     # the fold over every chunk
    if L >= 256:
        assert dropped > 0.1 * scale
