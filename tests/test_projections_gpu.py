"""The library call forms of the projections on the device: every ATen matrix product of the linears and of the mixer operator,
forward and backward, with operand shapes and strides, against the lists recorded before the products moved into projections.py
(host half and the recorder: test_projections_cpu.py)."""
import pytest
import torch

from test_projections_cpu import MatmulLog, linear_forms

pytestmark = pytest.mark.gpu


def spiral_forms(dev, ssi, switches, mp):
    """spiral_ssm on one mixer and spiral_ssm_pair on two, with the inner projections on the library (PAIR_OWN_MAX_ROWS 0), bf16, at
    the shape of test_spiral_pair_equals_two_single_operators_bit_for_bit_on_library_projections: spiral(8), d_model 256."""
    from diffma_amd.mamba import Mamba
    from diffma_amd.tools import spiral

    torch.manual_seed(7)
    n, B, d_model, dtype = 8, 1, 256, torch.bfloat16
    orders, inverses = spiral(n)
    mixers = [Mamba(d_model=d_model, d_state=16, token_list=orders[k], token_list_reversal=orders[k + 1], origina_list=inverses[k],
                    origina_list_reversal=inverses[k + 1]).to(dev) for k in (2, 4)]
    Din = mixers[0].d_inner
    xz = [torch.randn(B, n * n, 2 * Din, device=dev).to(dtype).requires_grad_(True) for _ in mixers]
    dy = [torch.randn(B, n * n, Din, device=dev).to(dtype) for _ in mixers]
    A = [-torch.exp(m.A_log.detach().float()) for m in mixers]
    forms = {}
    with mp.context() as mpc:
        mpc.setattr(switches, "PAIR_OWN_MAX_ROWS", 0)
        assert ssi.spiral_ssm_pair_supported(B, n * n, dtype, *mixers)
        m = mixers[0]
        with MatmulLog() as rec:
            y = ssi.spiral_ssm(xz[0], m.conv1d.weight, m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.dt_proj.bias, A[0], m.D, m.scan_index)
            y.backward(dy[0])
        forms["spiral_single"] = rec.log
        with MatmulLog() as rec:
            ys = ssi.spiral_ssm_pair(xz[0], xz[1], mixers[0], mixers[1], A[0], A[1])
            torch.autograd.backward(list(ys), dy)
        forms["spiral_pair"] = rec.log
    torch.cuda.synchronize()
    assert all(p.grad is not None for m in mixers for p in (m.x_proj.weight, m.dt_proj.weight))
    return forms


# recorded on an MI355X at commit 47d99b8 (the last one with the products inside selective_scan_interface.py)
_R, _T = lambda r, c, ld=None: ((r, c), (ld or c, 1)), lambda r, c: ((r, c), (1, r))          # a row-major matrix; a transposed view of one
GPU_FORMS = {
    "splitk_bias": [("aten.addmm.default", ((256,), (1,)), _R(196, 128), _T(128, 256)),
                    ("aten.mm.default", _R(196, 256, 264), _R(256, 128)),                      # dx: the gradient as it arrived
                    ("aten.mm.dtype", _T(256, 196), _R(196, 128))],                            # dW in fp32: its contiguous copy, transposed
    "splitk_nt": [],                                                                           # 256 rows: all three on dm_gemm
    "splitk_nt_library": [("aten.mm.default", _R(256, 128), _T(128, 256)),
                          ("aten.mm.default", _R(256, 256), _T(256, 128)),                     # dx = dy (W^T)^T on the transposed weight copy
                          ("aten.mm.dtype", _T(256, 256), _R(256, 128))],
    "pair": [("aten.mm.out", _R(196, 128), _T(128, 256), _R(196, 256))] * 2
            + [("aten.mm.out", _R(196, 256), _R(256, 128), _R(196, 128))] * 2
            + [("aten.mm.dtype", _T(256, 196), _R(196, 128))] * 2,
    # x_proj forward, dWx, du += dx_dbl @ Wx (dt_proj runs on its own kernels here): one product per mixer
    "spiral_single": [("aten.mm.default", _R(192, 512), _T(512, 48)),
                      ("aten.mm.dtype", _T(48, 192), _R(192, 512)),
                      ("aten.addmm_.default", _R(192, 512), _R(192, 48), _R(48, 512))],
    "spiral_pair": [("aten.mm.default", _R(192, 512), _T(512, 48))] * 2
                   + [("aten.mm.dtype", _T(48, 192), _R(192, 512))] * 2
                   + [("aten.addmm_.default", _R(192, 512), _R(192, 48), _R(48, 512))] * 2,
}


def test_the_linears_issue_the_recorded_library_calls(gpu, monkeypatch):
    """linear_splitk with a bias (196 x 128 -> 256); without one at 256 rows with LARGE_MIN_ROWS 256 and K12 off -- which dm_gemm
    takes whole, so once more with PAIR_OWN_MAX_ROWS 0, where the library's NT input gradient shows; linear_pair with
    PAIR_OWN_MAX_ROWS 0: the same ATen entries on the same shapes and strides as before the move."""
    from diffma_amd import projections as proj

    got = linear_forms(gpu, proj, proj, monkeypatch)
    assert got == {k: v for k, v in GPU_FORMS.items() if not k.startswith("spiral")}, got


def test_the_mixer_operator_issues_the_recorded_library_calls(gpu, monkeypatch):
    """spiral_ssm and spiral_ssm_pair with the inner projections on the library: per mixer the calls of before the move."""
    from diffma_amd import projections as proj
    from diffma_amd import selective_scan_interface as ssi

    got = spiral_forms(gpu, ssi, proj, monkeypatch)
    assert got == {k: v for k, v in GPU_FORMS.items() if k.startswith("spiral")}, got
