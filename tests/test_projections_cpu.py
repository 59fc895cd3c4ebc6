"""projections.route against the five predicates it replaced, and the library call forms the CPU can reach.

1. The decision table.  The oracle below is the five predicates of selective_scan_interface.py as they stood before projections.py
   existed, copied verbatim, and composed the way their call sites composed them.  Operands are stand-ins with the handful of
   attributes hip_ops.gemm_supported / gemm_large_supported read; the library's host-only dm_gemm_supported / dm_gemm_large_supported
   run for real.
2. The call forms: every ATen matrix product a linear issues, forward and backward, with operand shapes and strides, against a
   literal list recorded before the move (same file, device half: test_projections_gpu.py).
"""
import itertools
import sys

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


# =====================================================================================================================================
# 1. The decision table
# =====================================================================================================================================
# ---- the oracle: verbatim; the globals it reads are this module's, patched by the test together with the module under test ----
from diffma_amd import hip_ops                      # noqa: E402

PAIR_OWN_MAX_ROWS, LARGE_MIN_ROWS, LARGE_MIN_COLS, LARGE_MAX_K_NARROW, LARGE_DGRAD_NT = 3200, 12288, 1024, 1024, True


def _own_single(a, b, a_kmajor, b_kmajor, out_dtype=None):
    rows = a.shape[0]
    return (64 <= rows <= PAIR_OWN_MAX_ROWS and a.dim() == 2 and b.dim() == 2
            and hip_ops.gemm_supported(a, b, a_kmajor, b_kmajor, out_dtype))


def _own_large(a, b):
    M, K = a.shape
    N = b.shape[0]
    if M < LARGE_MIN_ROWS or N < LARGE_MIN_COLS or (N < 1024 and K > LARGE_MAX_K_NARROW):
        return False
    return hip_ops.gemm_large_supported(a, b)


def _large_dgrad_nt(dy2c):
    return LARGE_DGRAD_NT and dy2c.is_cuda and dy2c.shape[0] >= LARGE_MIN_ROWS and dy2c.dtype in (torch.bfloat16, torch.float16)


def _pair_use_own(rows, a, b, a_kmajor, b_kmajor, out_dtype=None):
    return rows <= PAIR_OWN_MAX_ROWS and hip_ops.gemm_supported(a, b, a_kmajor, b_kmajor, out_dtype)


def _inner_on_own(G, M, a, b, a_kmajor, b_kmajor, out_dtype=None):
    return G == 2 and _pair_use_own(M // 4, a, b, a_kmajor, b_kmajor, out_dtype)


class Mat:
    """A 2-D device matrix as far as the support checks look."""
    is_cuda = True

    def __init__(self, rows, cols, dtype, pad=0, ptr=0):
        self.shape, self.dtype, self._stride, self._ptr = (rows, cols), dtype, (cols + pad, 1), ptr

    def dim(self):
        return 2

    def stride(self, i):
        return self._stride[i]

    def data_ptr(self):
        return self._ptr


FORM = {"fwd": (True, True, None), "dgrad": (True, False, None), "wgrad": (False, False, F32)}


def _oracle(kind, caller, a, b, bias):
    """The route as the call sites of _LinearSplitKFn / _linear_dgrad / _linear_wgrad, _LinearPairFn and _SpiralSSMFn chose it."""
    M = a.shape[0]
    if caller == "pair":
        return "dm_gemm" if _pair_use_own(M, a, b, *FORM[kind]) else "library"
    if caller in ("inner_pair", "inner_single"):
        return "dm_gemm" if _inner_on_own(2 if caller == "inner_pair" else 1, M, a, b, *FORM[kind]) else "library"
    if kind == "fwd":
        if not bias and a.is_cuda and _own_single(a, b, True, True):
            return "dm_gemm"
        if not bias and a.is_cuda and _own_large(a, b):
            return "dm_gemm_large"
        return "library"
    if kind == "wgrad":
        return "dm_gemm" if not bias and _own_single(a, b, False, False, torch.float32) else "library"
    if not bias and _own_single(a, b, True, False):
        return "dm_gemm"
    if _large_dgrad_nt(a):
        wt = Mat(b.shape[1], b.shape[0], b.dtype)                  # wc.t().contiguous(): a fresh allocation
        return "dm_gemm_large" if _own_large(a, wt) else "library_nt"
    return "library"


ROWS = (1, 63, 64, 196, 3200, 3201, 12287, 12288, 12544, 100352)
WIDTHS = ((2048, 512), (512, 1024), (1024, 512), (2096, 512), (2090, 512), (64, 1024), (1000, 512))          # (N, K)
LAYOUTS = (dict(), dict(a=dict(pad=4)), dict(b=dict(pad=4)), dict(a=dict(ptr=8)), dict(b=dict(ptr=8)))     # row stride % 8, pointer % 16
PATCHES = ((None, None, None), ("hip_ops", "GEMM_LARGE", False), ("proj", "LARGE_DGRAD_NT", False), ("proj", "LARGE_MIN_COLS", 512),
           ("proj", "PAIR_OWN_MAX_ROWS", 0))
# every route the predicates can give per (product, caller): the sweep must show each of them, or it proves nothing about it
REACHABLE = {("fwd", "single"): {"dm_gemm", "dm_gemm_large", "library"},
             ("dgrad", "single"): {"dm_gemm", "dm_gemm_large", "library_nt", "library"},
             ("wgrad", "single"): {"dm_gemm", "library"},
             **{(k, c): {"dm_gemm", "library"} for k in FORM for c in ("pair", "inner_pair")},
             **{(k, "inner_single"): {"library"} for k in FORM}}


def _operands(kind, M, N, K, dt, layout):
    (ar, ac), (br, bc) = {"fwd": ((M, K), (N, K)), "dgrad": ((M, N), (N, K)), "wgrad": ((M, N), (M, K))}[kind]
    return Mat(ar, ac, dt, **layout.get("a", {})), Mat(br, bc, dt, **layout.get("b", {}))


def test_route_equals_the_five_predicates_on_the_whole_grid(monkeypatch):
    """3 products x 4 callers x 10 row counts x 7 widths x 3 dtypes x bias (the single linear's) x 5 layouts, under the default
    switches and with GEMM_LARGE off, LARGE_DGRAD_NT off, LARGE_MIN_COLS 512 and PAIR_OWN_MAX_ROWS 0: the same route everywhere, and
    every route a (product, caller) can take is taken somewhere in the sweep."""
    from diffma_amd import projections as proj

    me = sys.modules[__name__]
    seen = {key: set() for key in REACHABLE}
    n = 0
    for where, name, value in PATCHES:
        with monkeypatch.context() as mp:
            if where == "hip_ops":
                mp.setattr(hip_ops, name, value)
            elif where == "proj":
                mp.setattr(proj, name, value)
                mp.setattr(me, name, value)
            for kind, caller, M, (N, K), dt, layout in itertools.product(FORM, ("single", "pair", "inner_pair", "inner_single"), ROWS,
                                                                          WIDTHS, (BF16, F16, F32), LAYOUTS):
                a, b = _operands(kind, M, N, K, dt, layout)
                for bias in ((False, True) if caller == "single" else (False,)):
                    want = _oracle(kind, caller, a, b, bias)
                    got = proj.route(kind, caller, a, b, bias)
                    assert got == want, (name, value, kind, caller, M, N, K, dt, layout, bias, got, want)
                    seen[(kind, caller)].add(want)
                    n += 1
    assert n == 5 * 3 * 5 * 10 * 7 * 3 * 5
    assert seen == REACHABLE, {k: (v, REACHABLE[k]) for k, v in seen.items() if v != REACHABLE[k]}


def test_the_switches_are_not_reexported_by_the_operator_module():
    """A test that still patches them on selective_scan_interface must fail, not silently exercise the other route."""
    from diffma_amd import selective_scan_interface as ssi

    for name in ("PAIR_OWN_MAX_ROWS", "LARGE_MIN_ROWS", "LARGE_MIN_COLS", "LARGE_MAX_K_NARROW", "LARGE_DGRAD_NT"):
        with pytest.raises(AttributeError):
            getattr(ssi, name)


# =====================================================================================================================================
# 2. The library call forms
# =====================================================================================================================================
class MatmulLog(TorchDispatchMode):
    """Every ATen matrix product issued while active: (overload, (shape, stride) of each tensor operand, `out=` last)."""
    OPS = ("mm", "addmm", "addmm_", "bmm", "baddbmm")

    def __init__(self):
        super().__init__()
        self.log = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func.overloadpacket.__name__ in self.OPS:
            self.log.append((str(func), *((tuple(t.shape), tuple(t.stride())) for t in (*args, *kwargs.values()) if isinstance(t, torch.Tensor))))
        return func(*args, **kwargs)


def linear_forms(dev, lin, switches, mp):
    """The three linear cases, forward and backward, on `dev`: {case: log}.  lin: the module that has linear_splitk / linear_pair;
    switches: the one that has the thresholds; mp: a monkeypatch.  bf16 operands; the gradient that arrives is a column block of a
    wider buffer, so that the products that read it as it came differ from those that read its contiguous copy."""
    g = torch.Generator().manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(BF16).to(dev)

    def run(fn, *inputs):
        ins = [t.requires_grad_(True) for t in inputs]
        with MatmulLog() as rec:
            ys = fn(*ins)
            ys = ys if isinstance(ys, tuple) else (ys,)
            torch.autograd.backward(list(ys), [rnd(*y.shape[:-1], y.shape[-1] + 8)[..., :y.shape[-1]] for y in ys])
        assert all(t.grad is not None for t in ins)
        return rec.log

    forms = {"splitk_bias": run(lin.linear_splitk, rnd(196, 128), rnd(256, 128), rnd(256))}
    with mp.context() as m:
        m.setattr(switches, "LARGE_MIN_ROWS", 256)
        m.setattr(hip_ops, "GEMM_LARGE", False)
        forms["splitk_nt"] = run(lin.linear_splitk, rnd(256, 128), rnd(256, 128))
        m.setattr(switches, "PAIR_OWN_MAX_ROWS", 0)            # 256 rows lie inside dm_gemm's window: only without it does the library show
        forms["splitk_nt_library"] = run(lin.linear_splitk, rnd(256, 128), rnd(256, 128))
    with mp.context() as m:
        m.setattr(switches, "PAIR_OWN_MAX_ROWS", 0)
        forms["pair"] = run(lin.linear_pair, rnd(196, 128), rnd(196, 128), rnd(256, 128), rnd(256, 128))
    return forms


# recorded on a host without a device at commit 47d99b8 (the last one with the products inside selective_scan_interface.py)
_R, _T = lambda r, c, ld=None: ((r, c), (ld or c, 1)), lambda r, c: ((r, c), (1, r))          # a row-major matrix; a transposed view of one
CPU_FORMS = {
    "splitk_bias": [("aten.addmm.default", ((256,), (1,)), _R(196, 128), _T(128, 256)),
                    ("aten.mm.default", _R(196, 256, 264), _R(256, 128)),                      # dx: the gradient as it arrived
                    ("aten.mm.default", _T(256, 196), _R(196, 128))],                          # dW: its contiguous copy, transposed
    "splitk_nt": [("aten.mm.default", _R(256, 128), _T(128, 256)),
                  ("aten.mm.default", _R(256, 256, 264), _R(256, 128)),                        # (no NT form on the host)
                  ("aten.mm.default", _T(256, 256), _R(256, 128))],
    "splitk_nt_library": [("aten.mm.default", _R(256, 128), _T(128, 256)),
                          ("aten.mm.default", _R(256, 256, 264), _R(256, 128)),
                          ("aten.mm.default", _T(256, 256), _R(256, 128))],
    "pair": [("aten.mm.out", _R(196, 128), _T(128, 256), _R(196, 256))] * 2
            + [("aten.mm.out", _R(196, 256), _R(256, 128), _R(196, 128))] * 2
            + [("aten.mm.default", _T(256, 196), _R(196, 128))] * 2,
}


def test_the_linears_issue_the_recorded_library_calls_on_the_host(monkeypatch):
    """linear_splitk with a bias (196 x 128 -> 256), without one (256 rows, LARGE_MIN_ROWS 256, K12 off) and linear_pair
    (PAIR_OWN_MAX_ROWS 0) on host tensors: the same ATen entries on the same shapes and strides as before the move."""
    from diffma_amd import projections as proj

    assert linear_forms(torch.device("cpu"), proj, proj, monkeypatch) == CPU_FORMS
