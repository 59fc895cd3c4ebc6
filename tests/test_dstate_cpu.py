"""d_state 64 and 128 in the selective scans, the parts that need no GPU: the backward's channel groups, the ABI version and
the size of the dB/dC partial rows (include/diffma_hip.h, dm_scan_bwd_args: bytes = nseq * seqlen * ceil(dim / GC) * 2 * dstate * 4).
"""
import pytest

# channels per workgroup of the sequential backward: 4 waves of 64 lanes, 16 states per lane from d_state 32 on
GROUP_CHANNELS = {8: 256, 16: 256, 32: 128, 64: 64, 128: 32}


def test_abi_version_names_the_wide_scans():
    from diffma_amd import _lib

    assert _lib.load().dm_abi_version() >= 30
    assert _lib.CONSTANTS["DM_ABI_VERSION"] >= 30


@pytest.mark.parametrize("N", sorted(GROUP_CHANNELS))
def test_scan_bwd_group_channels(N):
    from diffma_amd import _lib

    lib = _lib.load()
    gc = lib.dm_scan_bwd_group_channels(N)
    assert gc > 0 and gc == GROUP_CHANNELS[N]
    # a launch the chunk-parallel kernel cannot take: forced sequential, and a sequence too short to cut
    assert lib.dm_scan_bwd_launch_group_channels(24, 1024, 196, N, _lib.DM_FLAG_SCAN_SEQUENTIAL) == gc
    assert lib.dm_scan_bwd_launch_group_channels(24, 1024, 16, N, 0) == gc
    if N != 16:                                    # the chunk-parallel kernel is d_state 16 only: the library never chooses it elsewhere
        assert lib.dm_scan_bwd_launch_group_channels(24, 1024, 196, N, 0) == gc


def test_scan_bwd_group_channels_of_an_absent_width():
    from diffma_amd import _lib, hip_ops

    assert _lib.load().dm_scan_bwd_group_channels(48) <= 0
    with pytest.raises(_lib.DiffmaHipError, match="not built for d_state=48"):
        hip_ops.scan_bwd_partial_shape(2, 21, 128, 48)


@pytest.mark.parametrize("N", [16, 32, 64, 128])
@pytest.mark.parametrize("S,L,Dm", [(2, 21, 128), (4, 40, 200), (6, 196, 1024), (1, 1, 1)])
def test_scan_bwd_partial_rows_follow_the_header_formula(S, L, Dm, N):
    from diffma_amd import _lib, hip_ops

    shape = hip_ops.scan_bwd_partial_shape(S, L, Dm, N, _lib.DM_FLAG_SCAN_SEQUENTIAL)
    gc = GROUP_CHANNELS[N]
    assert shape == (S, L, -(-Dm // gc), 2 * N)
    nbytes = 4
    for n in shape:
        nbytes *= n
    assert nbytes == S * L * -(-Dm // gc) * 2 * N * 4
    if Dm == 1024:                                 # the figures the header quotes per (sequence, step): 0.5 KB, 2 KB, 8 KB, 32 KB
        assert nbytes // (S * L) == {16: 512, 32: 2048, 64: 8192, 128: 32768}[N]
