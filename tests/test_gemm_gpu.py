"""K11 (csrc/gemm.hip: dm_gemm / dm_gemm_n / dm_gemm_supported) per element against fp64, and K12 (dm_gemm_large) exact on integers.

Hand-built dm_gemm_args structs go through the C ABI, so strides, view offsets, dtypes, the layout pair and `accumulate` are chosen by
the test; the wrappers (hip_ops.gemm / gemm_supported, linear_splitk, linear_pair, _own_pair) are tested on top of that.  The
reference is a plain torch fp64 matmul of the rounded 16-bit operands, computed on the CPU.

Buffers.  A, B and C are views inside larger device buffers.  Operand padding holds NaN: the columns past the contiguous extent when
ld exceeds the width (or the other half of the row when A is the right half of a [rows, 2 extent] buffer) and three rows before and
after the matrix -- a padding element that reaches a product poisons the result.  C starts as NaN where it is to be written (an
element never written fails; with accumulate = 1 it starts as the addend) and as a sentinel (7.0) in its row padding, in two rows
before and eight rows after the matrix and in the column blocks beside it when C is a column block of a wider buffer; the sentinel
must survive bit for bit.

Tile families.  gemm_launch_t takes the first of 128 x 128 / BK 64 and 128 x 64 / BK 64 whose grid has at least 256 workgroups
(a pair counts both structs), else 64 x 64 / BK 128.  `_family` restates that rule and every exact shape asserts the family it was
chosen for, so a change of the rule shows up as a test to re-aim.

Bounds.  u = unit roundoff of the C dtype (2^-8 bf16, 2^-11 fp16, 0 fp32), TINY = 2^-24 absolute for fp16 subnormals,
EPS32 = 2^-24.  None is taken from a measured error.

1. Exact on integers (zero tolerance).  Operands are integers in [-2, 2] in bf16 / fp16: every product and every partial sum is an
   integer of magnitude <= 4 Kc < 2^24, so the fp32 accumulator is exact in ANY summation order and under any internal rounding of
   the matrix pipe.  fp32 C must equal the fp64 product (torch.equal); 16-bit C must equal the fp64 product rounded ONCE to the dtype,
   ref.to(dtype): the kernel packs with round-to-nearest-even (v_cvt_pk_bf16_f32, (_Float16)) and so does torch; |ref| <= 4 * 2096 is
   below the fp16 maximum, and an integer below 2^24 rounds to 16 bits the same way from fp64 and from fp32.  With accumulate = 1
   the addend is integers in [-64, 64] (exact in both 16-bit types): the sum is still an exact fp32 integer, rounded once.
2. Random values.  A product of two bf16 or two fp16 values has at most 16 / 22 significant bits and an exponent far inside the fp32
   range: it is exact in fp32.  What remains is the accumulation: any order of Kc fp32 additions rounded to nearest errs by at most
   Kc EPS32 S, S = (|A| @ |B|) in fp64.  The internal rounding of the 16-bit MFMA's 32-term block is not documented in this
   repository; a truncating multi-operand adder loses at most 2 EPS32 of the largest term per term, so the bound takes twice that:
       E_acc = 2 Kc EPS32 S
       fp32 C:    |got - ref| <= E_acc
       16-bit C:  |got - ref| <= u |ref| + TINY + E_acc (1 + u)        (the final rounding acts on the computed value: u E_acc)
       accumulate = 1:  one more addition, E_acc + EPS32 (|c| + S) in place of E_acc, and u applies to |c + ref|.
   The same derivation covers a library GEMM with fp32 accumulation and a 16-bit result (section 5's unrouted cases); a bias adds one
   term: Kc + 1 and S + |b|.
   Value cases: randn; rows of A scaled by 2^-10 and 2^6 (S and |ref| differ by orders of magnitude between elements); for fp16 a
   block whose operands have magnitudes in [2^e-1, 2^e) with e = round((-15.2 - log2(Kc) / 2) / 2) >= -11, all NORMAL fp16 numbers,
   so that the outputs (about 0.58 * 2^2e * sqrt(Kc) = 2^-16) land in the fp16 subnormal range, which TINY covers.
3. dm_gemm_n: the `_n` entry is the single entry on args[0], args[1], ... in order; congruent neighbours share a grid.  The k order
   of an element's sum does not depend on the tile family, so pair and single launches agree bit for bit also where they select
   different families.
"""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CODE = {F32: 0, BF16: 1, F16: 2}
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
EPS32 = 2.0 ** -24
UNIT = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
TINY = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -24}
DM_OK, DM_ERR_ARG, DM_ERR_LAYOUT = 0, -1, -2
SENT = 7.0
NAN = float("nan")
KM = [(1, 1), (1, 0), (0, 1), (0, 0)]                  # (a_kmajor, b_kmajor)
MODES = ["contig", "padded", "half"]                   # see _operand / _cbuf
T64, T128x64, T128 = (64, 64, 128), (128, 64, 64), (128, 128, 64)
WORST = {}                                             # (operand dtype, C dtype, what) -> worst measured ratio, printed per test


def _lib():
    from diffma_amd import _lib as L

    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw(name, a):
    """Status code of one C-ABI call (no exception: the argument-check cases compare it)."""
    return int(getattr(_lib().load(), name)(ctypes.byref(a), _stream()))


def _raw_n(name, structs):
    arr = (type(structs[0]) * len(structs))(*structs)
    return int(getattr(_lib().load(), name)(ctypes.cast(arr, ctypes.c_void_p), len(structs), _stream()))


def _err():
    return _lib().load().dm_last_error().decode()


def _family(P, Q, n=1):
    """(BM, BN, BK) by the rule of gemm_launch_t (csrc/gemm.hip); n = 2 for a pair."""
    wgs = lambda bm, bn: n * -(-P // bm) * -(-Q // bn)
    return T128 if wgs(128, 128) >= 256 else T128x64 if wgs(128, 64) >= 256 else T64


def _ceil8(n):
    return (n + 7) // 8 * 8


def _operand(gpu, stored, mode, pad):
    """The stored matrix [R, W] as a view inside a NaN-filled buffer with three spare rows on either side.  contig: row stride W;
    padded: W + pad; half: the right half of a [R, 2 W] buffer."""
    R, W = stored.shape
    ld = {"contig": W, "padded": W + pad, "half": 2 * W}[mode]
    buf = torch.full((R + 6, ld), NAN, dtype=stored.dtype, device=gpu)
    view = buf[3:3 + R, ld - W:] if mode == "half" else buf[3:3 + R, :W]
    view.copy_(stored)
    assert view.data_ptr() % 16 == 0 and view.stride() == (ld, 1)
    return buf, view


def _cbuf(gpu, P, Q, cdt, mode, init=None):
    """C [P, Q] inside a sentinel-filled buffer, two rows before it and eight after.  contig: row stride Q; padded: Q + 4 (C strides
    need only % 4); half: columns [8, 8 + Q) of rows Q + 24 wide.  The view holds NaN, or `init` (the addend of accumulate = 1)."""
    ldc, c0 = {"contig": (Q, 0), "padded": (Q + 4, 0), "half": (Q + 24, 8)}[mode]
    buf = torch.full((P + 10, ldc), SENT, dtype=cdt, device=gpu)
    view = buf[2:2 + P, c0:c0 + Q]
    if init is None:
        view.fill_(NAN)
    else:
        view.copy_(init)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _untouched(buf, view):
    chk = buf.clone()
    chk.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(SENT)
    return bool((chk == SENT).all())


def _args(av, bv, cv, P, Q, Kc, akm, bkm, acc=0):
    a = _lib().dm_gemm_args()
    a.P, a.Q, a.Kc = P, Q, Kc
    a.ab_dtype, a.c_dtype = CODE[av.dtype], CODE[cv.dtype]
    a.a_kmajor, a.b_kmajor, a.accumulate = akm, bkm, acc
    a.a, a.b, a.c = av.data_ptr(), bv.data_ptr(), cv.data_ptr()
    a.lda, a.ldb, a.ldc = av.stride(0), bv.stride(0), cv.stride(0)
    return a


def _setup(gpu, A, B, akm, bkm, cdt, mode="padded", c0=None):
    """Device buffers and the struct of C (+)= A @ B for the LOGICAL operands A [P, Kc], B [Kc, Q] (16-bit, host or device): each is
    stored k-major ([rows][Kc]) or row-major ([Kc][rows]) as the layout pair says.  Strided: lda = extent + 8, ldb = extent + 16."""
    P, Kc = A.shape
    Q = B.shape[1]
    d = dict(P=P, Q=Q, Kc=Kc)
    d["abuf"], d["a"] = _operand(gpu, A if akm else A.t(), mode, 8)
    d["bbuf"], d["b"] = _operand(gpu, B.t() if bkm else B, "padded" if mode == "half" else mode, 16)
    d["cbuf"], d["c"] = _cbuf(gpu, P, Q, cdt, mode, c0)
    d["args"] = _args(d["a"], d["b"], d["c"], P, Q, Kc, akm, bkm, 0 if c0 is None else 1)
    return d


def _same(name, got, want):
    """Bit-for-bit equality of values (a NaN in got -- an element the kernel never wrote -- fails)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = ~(got == want)
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {want.numel()} elements differ; first at row {i // want.shape[1]} column "
                             f"{i % want.shape[1]}: got {float(got.flatten()[i])} want {float(want.flatten()[i])}")


def _check(name, got, ref, tol, key=None, E=None):
    """Per-element |got - ref| <= tol (NaN in got fails).  key = (operand dtype, C dtype, tag): record the worst err / tol, and the
    worst err / E where E (the accumulation share of the bound) is given."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    if key is not None:
        ok = tol > 0
        for what, den in (("err/tol", tol),) + ((("err/E_acc", E),) if E is not None else ()):
            k = key + (what,)
            WORST[k] = max(WORST.get(k, 0.0), float((err[ok] / den[ok]).nan_to_num(nan=1e30).max()))
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {ref.numel()} elements out of bound; first at flat {i}: "
                             f"got {float(got.flatten()[i])} ref {float(ref.flatten()[i])} tol {float(tol.flatten()[i])}")


def _report():
    """The figures measured so far (shown by pytest -s / -rP; nothing is asserted on them)."""
    for k in sorted(WORST, key=str):
        print(f"worst {k[3]} [{k[2]}] operands {NAME[k[0]]} C {NAME[k[1]]}: {WORST[k]:.4f}")


def _bound(ref, S, Kc, cdt, c0=None, extra_terms=0):
    """(reference, per-element tolerance, E) of the module docstring's section 2; c0: the addend of accumulate = 1."""
    E = 2 * (Kc + extra_terms) * EPS32 * S
    if c0 is not None:
        E = E + EPS32 * (c0.abs() + S)
        ref = ref + c0
    u = UNIT[cdt]
    return ref, u * ref.abs() + TINY[cdt] + E * (1 + u), E


# =====================================================================================================================================
# 1. exact on integers
# =====================================================================================================================================
@functools.lru_cache(maxsize=4)
def _int_case(P, Q, Kc, seed=0):
    """Integer operands in [-2, 2], an addend in [-64, 64] and the fp64 product, computed once per shape on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + P + 3 * Q + 7 * Kc)
    A = torch.randint(-2, 3, (P, Kc), generator=g).double()
    B = torch.randint(-2, 3, (Kc, Q), generator=g).double()
    C0 = torch.randint(-64, 65, (P, Q), generator=g).double()
    ref = A @ B
    assert float(ref.abs().max()) <= 4 * Kc < 2 ** 24 and float((ref + C0).abs().max()) < 65504
    return A, B, C0, ref


def _exact_one(gpu, A, B, want, akm, bkm, mode, c0=None, entry="dm_gemm"):
    """One launch on integer operands; `want` (device, C dtype) must come back bit for bit, the sentinel around it untouched."""
    from diffma_amd import hip_ops

    d = _setup(gpu, A, B, akm, bkm, want.dtype, mode, c0)
    what = (entry, d["P"], d["Q"], d["Kc"], NAME[A.dtype], NAME[want.dtype], akm, bkm, mode, c0 is not None)
    if entry == "dm_gemm":
        sup = _lib().load().dm_gemm_supported(d["P"], d["Q"], d["Kc"], akm, bkm, CODE[A.dtype], CODE[want.dtype])
        assert sup == 1 and hip_ops.gemm_supported(d["a"], d["b"], bool(akm), bool(bkm), want.dtype), what
    rc = _raw(entry, d["args"])
    assert rc == DM_OK, (what, rc, _err())
    torch.cuda.synchronize()
    _same(str(what), d["c"], want)
    assert _untouched(d["cbuf"], d["c"]), (what, "written outside C")
    assert torch.equal(d["a"], (A if akm else A.t()).to(gpu)) and torch.equal(d["b"], (B.t() if bkm else B).to(gpu)), (what, "operands are read-only")
    return d


# P, Q, Kc, the family the shape is aimed at, layout pairs ("all": P rounded up to a multiple of 8 where A is row-major)
EXACT_SHAPES = [
    (8, 8, 8, T64, "all"),                  # the smallest the predicate takes
    (72, 24, 136, T64, "all"),              # an 8-row tail tile, Q < 64, Kc = 128 + 8
    (200, 2096, 72, T64, "all"),            # Mamba-2 in_proj forward width: 48-column tail tile
    (196, 2096, 512, T64, "akm"),           # ... at the real row count (k-major A only)
    (200, 512, 2096, T64, "all"),           # Mamba-2 in_proj input gradient: Kc % 128 = 48
    (2096, 512, 197, T64, "rm"),            # both operands row-major: an odd contraction is legal only there
    (64, 64, 1, T64, "rm"),                 # Kc = 1
    (196, 1024, 64, T64, "all"),            # Kc is half a BK
    (1288, 1544, 72, T128x64, "all"),       # 11 x 25 = 275 workgroups (11 x 13 = 143 for 128 x 128); 8-row and 8-column tail tiles, Kc = 64 + 8
    (2056, 2096, 72, T128, "all"),          # 17 x 17 = 289 workgroups; 8-row tail, 48-column tail
]
ACC_SHAPES = {(8, 8, 8), (72, 24, 136), (1288, 1544, 72), (2056, 2096, 72)}      # accumulate = 1: every family, both C dtypes


@pytest.mark.parametrize("P,Q,Kc,fam,lay", EXACT_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in EXACT_SHAPES])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_gemm_exact_on_integers(gpu, dt, P, Q, Kc, fam, lay):
    """Section 1 of the module docstring: {bf16, fp16} x C in {fp32, operand dtype} x the layout pairs x {contiguous, padded rows,
    A the right half of a wider buffer with C a column block}, zero tolerance; accumulate = 1 on one shape per tile family."""
    P8 = _ceil8(P)
    A, B, C0, ref = _int_case(P8, Q, Kc)
    Ad, Bd = A.to(dt).to(gpu), B.to(dt).to(gpu)
    pairs = {"all": KM, "akm": [(1, 1), (1, 0)], "rm": [(0, 0)]}[lay]
    want, want_acc, c0 = {}, {}, {}
    for cdt in (F32, dt):
        want[cdt] = ref.to(cdt).to(gpu)
        assert torch.equal(want[cdt].cpu(), ref.float().to(cdt))                    # rounding through fp32 is the same single rounding
        if (P, Q, Kc) in ACC_SHAPES:
            c0[cdt] = C0.to(cdt).to(gpu)
            want_acc[cdt] = (ref + C0).to(cdt).to(gpu)
    for akm, bkm in pairs:
        Pe = P if akm else P8
        assert _family(Pe, Q) == fam, (Pe, Q, _family(Pe, Q))
        for cdt in (F32, dt):
            for mode in MODES:
                _exact_one(gpu, Ad[:Pe], Bd, want[cdt][:Pe], akm, bkm, mode)
            if (P, Q, Kc) in ACC_SHAPES:
                _exact_one(gpu, Ad[:Pe], Bd, want_acc[cdt][:Pe], akm, bkm, "padded", c0=c0[cdt][:Pe])
                _exact_one(gpu, Ad[:Pe], Bd, want_acc[cdt][:Pe], akm, bkm, "half", c0=c0[cdt][:Pe])


def test_gemm_integer_case_rounds_on_ties():
    """The integer construction exercises the rounding rule of the 16-bit C: with Kc = 2096 the product holds hundreds of values that
    are exact ties in bf16 (odd integers in [256, 512), odd multiples of 2 in [512, 1024)), and ref.to(bf16) rounds them to even."""
    _, _, _, ref = _int_case(200, 512, 2096)
    v = ref.abs()
    ulp = torch.exp2(torch.floor(torch.log2(v.clamp(min=1))) - 7)                   # bf16 spacing at |v|
    ties = (v >= 256) & (torch.remainder(v, ulp) == ulp / 2)
    assert int(ties.sum()) >= 100, int(ties.sum())
    r = ref.to(BF16).double().abs()
    assert bool((torch.remainder(r[ties] / ulp[ties], 2) == 0).all())


# =====================================================================================================================================
# 2. random values, per element
# =====================================================================================================================================
def _rand_logical(P, Q, Kc, dt, case, g, a_scale=1.0, b_scale=1.0):
    """Logical A [P, Kc], B [Kc, Q] rounded to dt.  case: randn | scaled | subnormal (module docstring, section 2)."""
    A = torch.randn(P, Kc, generator=g) * a_scale
    B = torch.randn(Kc, Q, generator=g) * b_scale
    blk = None
    if case == "scaled":
        A[0::7] *= 2.0 ** -10
        A[3::7] *= 2.0 ** 6
    elif case == "subnormal":
        e = round((-15.2 - 0.5 * math.log2(Kc)) / 2)
        assert e >= -11
        r0, c0 = (8 if P >= 24 else 0), (8 if Q >= 24 else 0)
        r1, c1 = r0 + min(16, P - r0), c0 + min(16, Q - c0)
        mag = lambda *s: (0.5 + 0.5 * torch.rand(*s, generator=g)) * torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0) * 2.0 ** e
        A[r0:r1] = mag(r1 - r0, Kc)
        B[:, c0:c1] = mag(Kc, c1 - c0)
        blk = (slice(r0, r1), slice(c0, c1))
    A, B = A.to(dt), B.to(dt)
    if blk is not None:
        assert float(A[blk[0]].abs().min()) >= 2.0 ** -14 and float(B[:, blk[1]].abs().min()) >= 2.0 ** -14      # normal fp16 operands
    return A, B, blk


def _rand_product(gpu, A, B, akm, bkm, cdts, mode="padded", acc_seed=None):
    """C (+)= A @ B on the device for every C dtype in cdts, each element against fp64 within the derived bound."""
    P, Kc = A.shape
    Q = B.shape[1]
    ref = A.double() @ B.double()
    S = A.double().abs() @ B.double().abs()
    for cdt in cdts:
        c0 = None
        if acc_seed is not None:
            c0 = (torch.randn(P, Q, generator=torch.Generator().manual_seed(acc_seed)) * 2).to(cdt)
        d = _setup(gpu, A, B, akm, bkm, cdt, mode, c0)
        rc = _raw("dm_gemm", d["args"])
        assert rc == DM_OK, (rc, _err())
        torch.cuda.synchronize()
        r, tol, E = _bound(ref, S, Kc, cdt, None if c0 is None else c0.double())
        _check(f"{P}x{Q}x{Kc} {NAME[A.dtype]}->{NAME[cdt]} kmajor {akm}{bkm} acc {c0 is not None}", d["c"], r, tol,
               (A.dtype, cdt, "dm_gemm accumulate" if c0 is not None else "dm_gemm"), E if cdt == F32 and c0 is None else None)
        assert _untouched(d["cbuf"], d["c"])
    return ref


LINEAR = [(512, 2096), (512, 2048), (1024, 512), (1024, 64)]


@pytest.mark.parametrize("M,K,N", [(M, K, N) for K, N in LINEAR for M in (196, 200)] + [(72, 136, 24), (8, 8, 8)])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_gemm_random_within_derived_bound(gpu, dt, M, K, N):
    """Section 2: the three products of a Linear layer (forward, input gradient, fp32 weight gradient) and, where M is a multiple of
    8, the forward with A row-major (the layout pair nothing in the package uses); 16-bit and fp32 C; the accumulating form on the
    input gradient.  Value cases: randn, rows of A scaled by 2^-10 and 2^6, and for fp16 a block with subnormal outputs."""
    for ci, case in enumerate(("randn", "scaled") + (("subnormal",) if dt == F16 else ())):
        g = torch.Generator().manual_seed(7 * M + K + N + ci)
        ws = K ** -0.5
        prods = [("fwd", M, N, K, 1, 1, 1.0, ws, (dt, F32)), ("dgrad", M, K, N, 1, 0, 1.0, ws, (dt, F32)), ("wgrad", N, K, M, 0, 0, 1.0, 1.0, (F32,))]
        if M % 8 == 0:
            prods.append(("fwd-a-rowmajor", M, N, K, 0, 1, 1.0, ws, (dt, F32)))
        for name, P, Q, Kc, akm, bkm, sa, sb, cdts in prods:
            A, B, blk = _rand_logical(P, Q, Kc, dt, case, g, sa, sb)
            ref = _rand_product(gpu, A, B, akm, bkm, cdts)
            if blk is not None:
                sub = ref[blk].abs()
                assert float(((sub < 2.0 ** -14) & (sub > 0)).double().mean()) > 0.5, (name, "the block's outputs are not subnormal")
            if name == "dgrad":
                _rand_product(gpu, A, B, akm, bkm, (dt, F32), acc_seed=M + ci)
    _report()


# =====================================================================================================================================
# 3. dm_gemm_n
# =====================================================================================================================================
def _int_setup(gpu, P, Q, Kc, dt, cdt, akm, bkm, seed):
    A, B, _, ref = _int_case(P, Q, Kc, seed)
    d = _setup(gpu, A.to(dt), B.to(dt), akm, bkm, cdt, "padded")
    d["want"] = ref.to(cdt).to(gpu)
    return d


def _exact_after(d, what):
    _same(str(what), d["c"], d["want"])
    assert _untouched(d["cbuf"], d["c"]), (what, "written outside C")


@pytest.mark.parametrize("P,Q,Kc,single,pair", [(392, 2048, 72, T64, T128x64), (1288, 1544, 72, T128x64, T128)], ids=["64-to-128x64", "128x64-to-128x128"])
def test_gemm_n_congruent_pair_is_exact_and_equals_two_single_launches(gpu, P, Q, Kc, single, pair):
    """Two congruent structs share one grid, whose size selects ANOTHER tile family than a single launch of the same shape: both
    results exact, and bit for bit those of two single launches."""
    assert _family(P, Q) == single and _family(P, Q, 2) == pair
    for dt, cdt in ((BF16, BF16), (F16, F32)):
        for akm, bkm in KM:
            two = [_int_setup(gpu, P, Q, Kc, dt, cdt, akm, bkm, s) for s in (1, 2)]
            one = [_int_setup(gpu, P, Q, Kc, dt, cdt, akm, bkm, s) for s in (1, 2)]
            rc = _raw_n("dm_gemm_n", [d["args"] for d in two])
            assert rc == DM_OK, (rc, _err())
            for d in one:
                assert _raw("dm_gemm", d["args"]) == DM_OK, _err()
            torch.cuda.synchronize()
            for k in (0, 1):
                _exact_after(two[k], ("pair", k, NAME[dt], akm, bkm))
                _exact_after(one[k], ("single", k, NAME[dt], akm, bkm))
                assert torch.equal(two[k]["c"], one[k]["c"])


def test_gemm_n_incongruent_pair_and_three_structs(gpu):
    """Structs of different P cannot share a grid and run one after the other; n = 3 is a congruent pair plus a single.  Every
    result exact."""
    for dt, cdt in ((BF16, F32), (F16, F16)):
        for akm, bkm in KM:
            ds = [_int_setup(gpu, 392, 2048, 72, dt, cdt, akm, bkm, 1), _int_setup(gpu, 200, 2048, 72, dt, cdt, akm, bkm, 2)]
            assert _raw_n("dm_gemm_n", [d["args"] for d in ds]) == DM_OK, _err()
            ts = [_int_setup(gpu, 392, 2048, 72, dt, cdt, akm, bkm, 1), _int_setup(gpu, 392, 2048, 72, dt, cdt, akm, bkm, 2),
                  _int_setup(gpu, 72, 24, 136, dt, cdt, akm, bkm, 3)]
            assert _raw_n("dm_gemm_n", [d["args"] for d in ts]) == DM_OK, _err()
            torch.cuda.synchronize()
            for k, d in enumerate(ds + ts):
                _exact_after(d, ("n", k, NAME[dt], akm, bkm))


def test_gemm_n_checks_every_struct_like_a_single_call(gpu):
    """Two structs congruent in every size and stride, one with `a` starting 8 bytes into its 16-byte aligned place: the single
    entry refuses it (DM_ERR_LAYOUT).  Valid struct first: that status, the first output bit for bit that of a single call, the
    second output untouched; invalid struct first: that status and nothing written."""
    P, Q, Kc = 392, 2048, 72
    mk = lambda s: _int_setup(gpu, P, Q, Kc, BF16, BF16, 1, 1, s)
    ref = mk(1)
    assert _raw("dm_gemm", ref["args"]) == DM_OK
    lone = mk(2)
    lone["args"].a += 8
    assert _raw("dm_gemm", lone["args"]) == DM_ERR_LAYOUT
    clean = lambda d: bool(torch.isnan(d["c"]).all()) and _untouched(d["cbuf"], d["c"])
    for order in ((0, 1), (1, 0)):
        ds = [mk(1), mk(2)]
        ds[1]["args"].a += 8
        assert ds[1]["args"].a % 16 == 8
        rc = _raw_n("dm_gemm_n", [ds[k]["args"] for k in order])
        torch.cuda.synchronize()
        assert rc == DM_ERR_LAYOUT and _err(), (order, rc)
        assert clean(ds[1]) and clean(lone), order
        if order == (0, 1):
            assert torch.equal(ds[0]["c"], ref["c"]) and _untouched(ds[0]["cbuf"], ds[0]["c"])
            _exact_after(ds[0], "valid struct first")
        else:
            assert clean(ds[0])


# =====================================================================================================================================
# 4. argument checks and the three predicates
# =====================================================================================================================================
def test_gemm_argument_checks(gpu):
    """Refusals by return code, nothing launched: dm_gemm_supported says 0 where the case lies in the predicate's domain, dm_gemm
    returns the stated status and leaves a message of its own, and C keeps its sentinel.  The buffers are far larger than any
    variant would touch.  (P > 64 * 65535 is left out: a test must not be one bug away from a launch over a buffer that is not
    there.)"""
    L = _lib()
    lib = L.load()
    abuf, bbuf = torch.zeros(64, 64, dtype=BF16, device=gpu), torch.zeros(64, 64, dtype=BF16, device=gpu)
    cbuf = torch.full((64, 64), SENT, dtype=F32, device=gpu)
    base = dict(P=16, Q=16, Kc=16, ab_dtype=CODE[BF16], c_dtype=CODE[BF16], a_kmajor=1, b_kmajor=1, accumulate=0,
                a=abuf.data_ptr(), b=bbuf.data_ptr(), c=cbuf.data_ptr(), lda=32, ldb=32, ldc=32)

    def args(**kw):
        a = L.dm_gemm_args()
        for k, v in {**base, **kw}.items():
            setattr(a, k, v)
        return a

    ok_c = torch.full((64, 64), SENT, dtype=F32, device=gpu)
    for akm, bkm in KM:                                            # the accepting side: the unmodified struct in every layout pair
        assert _raw("dm_gemm", args(a_kmajor=akm, b_kmajor=bkm, c=ok_c.data_ptr())) == DM_OK, _err()
        assert lib.dm_gemm_supported(16, 16, 16, akm, bkm, CODE[BF16], CODE[BF16]) == 1
    assert int(lib.dm_gemm(None, _stream())) == DM_ERR_ARG

    table = []                                                     # (what, overrides, status, in the predicate's domain)
    table += [("Q % 8", dict(Q=12), DM_ERR_ARG, True), ("Q % 8, both row-major", dict(Q=20, a_kmajor=0, b_kmajor=0), DM_ERR_ARG, True)]
    table += [(f"Kc % 8, kmajor {p}", dict(Kc=12, a_kmajor=p[0], b_kmajor=p[1]), DM_ERR_ARG, True) for p in KM[:3]]
    table += [(f"odd Kc, kmajor {p}", dict(Kc=13, a_kmajor=p[0], b_kmajor=p[1]), DM_ERR_ARG, True) for p in KM[:3]]
    table += [(f"P % 8, A row-major, b_kmajor {b}", dict(P=12, a_kmajor=0, b_kmajor=b), DM_ERR_ARG, True) for b in (0, 1)]
    table += [("fp32 operands", dict(ab_dtype=CODE[F32], c_dtype=CODE[F32]), DM_ERR_ARG, True),
              ("fp32 operands, 16-bit C", dict(ab_dtype=CODE[F32]), DM_ERR_ARG, True),
              ("bf16 operands, fp16 C", dict(c_dtype=CODE[F16]), DM_ERR_ARG, True),
              ("fp16 operands, bf16 C", dict(ab_dtype=CODE[F16]), DM_ERR_ARG, True),
              ("unknown operand dtype", dict(ab_dtype=3, c_dtype=3), DM_ERR_ARG, True)]
    table += [(f"{f} = {v}", {f: v}, DM_ERR_ARG, True) for f in ("P", "Q", "Kc") for v in (0, -8)]
    table += [(f"null {f}", {f: 0}, DM_ERR_ARG, False) for f in ("a", "b", "c")]
    table += [("lda below Kc", dict(lda=8), DM_ERR_LAYOUT, False), ("ldb below Kc", dict(ldb=8), DM_ERR_LAYOUT, False),
              ("lda below P, A row-major", dict(P=24, a_kmajor=0, lda=16), DM_ERR_LAYOUT, False),
              ("ldb below Q, B row-major", dict(Q=24, b_kmajor=0, ldb=16), DM_ERR_LAYOUT, False),
              ("lda % 8", dict(lda=20), DM_ERR_LAYOUT, False), ("ldb % 8", dict(ldb=20), DM_ERR_LAYOUT, False),
              ("ldc below Q", dict(ldc=8), DM_ERR_LAYOUT, False), ("ldc % 4", dict(ldc=18), DM_ERR_LAYOUT, False),
              ("ldc % 4, fp32 C", dict(ldc=18, c_dtype=CODE[F32]), DM_ERR_LAYOUT, False)]
    table += [(f"{f} misaligned by 8 bytes", {f: base[f] + 8}, DM_ERR_LAYOUT, False) for f in ("a", "b", "c")]
    for what, kw, status, in_domain in table:
        a = args(**kw)
        if in_domain:
            assert lib.dm_gemm_supported(a.P, a.Q, a.Kc, a.a_kmajor, a.b_kmajor, a.ab_dtype, a.c_dtype) == 0, what
        assert int(lib.dm_gemm(None, _stream())) == DM_ERR_ARG and _err() == "dm_gemm: null args"       # (a known message to replace)
        assert _raw("dm_gemm", a) == status, (what, _err())
        msg = _err()
        assert msg.startswith("dm_gemm: ") and msg != "dm_gemm: null args", (what, msg)
        assert _raw_n("dm_gemm_n", [a]) == status, what
    torch.cuda.synchronize()
    assert bool((cbuf == SENT).all()), "a refused call wrote to C"


def test_gemm_supported_wrapper_agrees_with_the_entry(gpu):
    """hip_ops.gemm_supported adds the layout half of check_gemm to dm_gemm_supported: false for a column stride != 1, a row stride
    that is not a multiple of 8, a misaligned base pointer, fp32 and mixed dtypes (true for the same operands without the defect;
    section 1 asserts agreement on every supported case).  hip_ops.gemm with a C row stride that is not a multiple of 4 raises."""
    from diffma_amd import hip_ops

    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=gpu)
    a, b = z(16, 16), z(16, 16)
    for akm, bkm in KM:
        assert hip_ops.gemm_supported(a, b, bool(akm), bool(bkm)) and hip_ops.gemm_supported(a, b, bool(akm), bool(bkm), F32)
        assert not hip_ops.gemm_supported(z(16, 32)[:, ::2], b, bool(akm), bool(bkm))
        assert not hip_ops.gemm_supported(a, z(16, 32)[:, ::2], bool(akm), bool(bkm))
        assert not hip_ops.gemm_supported(z(16, 20)[:, :16], b, bool(akm), bool(bkm))
        assert not hip_ops.gemm_supported(a, z(16, 20)[:, :16], bool(akm), bool(bkm))
        assert hip_ops.gemm_supported(z(16, 24)[:, :16], z(16, 32)[:, 16:], bool(akm), bool(bkm))
        off = z(16 * 16 + 8)[4:4 + 256].view(16, 16)
        assert off.data_ptr() % 16 == 8
        assert not hip_ops.gemm_supported(off, b, bool(akm), bool(bkm)) and not hip_ops.gemm_supported(a, off, bool(akm), bool(bkm))
        assert not hip_ops.gemm_supported(z(16, 16, dt=F32), z(16, 16, dt=F32), bool(akm), bool(bkm))
        assert not hip_ops.gemm_supported(a, z(16, 16, dt=F16), bool(akm), bool(bkm))
    assert not hip_ops.gemm_supported(z(16, 16), z(12, 16), True, True)            # Q % 8: the entry's own predicate
    out = torch.full((16, 18), SENT, dtype=BF16, device=gpu)
    with pytest.raises(_lib().DiffmaHipError):
        hip_ops.gemm(a, b, out=out[:, :16])
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# =====================================================================================================================================
# 5. routing at the Mamba-2 widths
# =====================================================================================================================================
def _record(monkeypatch):
    """Every C-ABI launch the wrappers make, as (single | n, entry point name)."""
    L = _lib()
    names, real, real_n = [], L.call, L.call_n
    monkeypatch.setattr(L, "call", lambda name, a, st: (names.append(("single", name)), real(name, a, st))[1])
    monkeypatch.setattr(L, "call_n", lambda name, a, st: (names.append(("n", name)), real_n(name, a, st))[1])
    return names


def _linear_case(gpu, rows, K, N, dt, seed, bias=False):
    """16-bit x [1, rows, K] and dy, fp32 master W [N, K] (and bias): device leaves, and fp64 autograd on the rounded operands."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, rows, K, generator=g).to(dt)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) if bias else None
    dy = torch.randn(1, rows, N, generator=g).to(dt)
    x64 = x.double().requires_grad_(True)
    W64 = W.to(dt).double().requires_grad_(True)
    b64 = b.to(dt).double() if bias else None
    y64 = x64 @ W64.t() + (b64 if bias else 0.0)
    y64.backward(dy.double())
    xa, Wa, da = x.double().abs()[0], W.to(dt).double().abs(), dy.double().abs()[0]
    r = dict(y=y64.detach()[0], dx=x64.grad[0], dW=W64.grad, S_y=xa @ Wa.t() + (b64.abs() if bias else 0.0), S_dx=da @ Wa, S_dW=da.t() @ xa,
             db=dy.double()[0].sum(0), S_db=da.sum(0))
    leaves = [x.to(gpu).requires_grad_(True), W.to(gpu).requires_grad_(True), b.to(gpu).requires_grad_(True) if bias else None]
    return leaves, dy.to(gpu), r


def _linear_verify(name, dt, r, y, dx, dW, rows, K, N, dW_dt, bias=False):
    tag = "linear " + name.split()[0]
    _check(f"{name} y", y[0], *_bound(r["y"], r["S_y"], K, dt, extra_terms=int(bias))[:2], key=(dt, dt, tag))
    _check(f"{name} x.grad", dx[0], *_bound(r["dx"], r["S_dx"], N, dt)[:2], key=(dt, dt, tag))
    ref, tol, E = _bound(r["dW"], r["S_dW"], rows, dW_dt)
    _check(f"{name} W.grad", dW, ref, tol, key=(dt, dW_dt, tag), E=E if dW_dt == F32 else None)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_linear_splitk_runs_dm_gemm_at_the_mamba2_width(gpu, monkeypatch, dt):
    """in_proj of the Mamba-2 mixer at hidden size 512 (512 -> 2096 = 2 * 1024 + 2 * 16 + 16), one sample of 196 tokens, fp32
    master weight, autocast: the forward and both gradients run on dm_gemm (three single launches), each within the section-2
    bounds of fp64 autograd on the rounded operands; W.grad is the kernel's fp32 output (the cast to the weight dtype is fp32 to
    fp32)."""
    from diffma_amd import projections as proj

    names = _record(monkeypatch)
    (x, W, _), dy, r = _linear_case(gpu, 196, 512, 2096, dt, 11)
    with torch.autocast("cuda", dtype=dt):
        y = proj.linear_splitk(x, W)
    y.backward(dy)
    torch.cuda.synchronize()
    assert names == [("single", "dm_gemm")] * 3, names
    assert y.dtype == dt and x.grad.dtype == dt and W.grad.dtype == F32
    _linear_verify("own", dt, r, y, x.grad, W.grad, 196, 512, 2096, F32)
    _report()


@pytest.mark.parametrize("case", ["rows63", "rows_max_plus_1", "bias", "width2090"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_linear_splitk_leaves_dm_gemm_alone_outside_its_gate(gpu, monkeypatch, dt, case):
    """The same call with 63 rows, with PAIR_OWN_MAX_ROWS + 1 rows, with a bias, and at a width that is not a multiple of 8 records
    no dm_gemm; the library computes the products (fp32 accumulation, 16-bit results, at most one more rounding of W.grad to 16
    bits), so the 16-bit bound of section 2 holds for all three."""
    from diffma_amd import projections as proj

    rows = {"rows63": 63, "rows_max_plus_1": proj.PAIR_OWN_MAX_ROWS + 1}.get(case, 196)
    N = 2090 if case == "width2090" else 2096
    bias = case == "bias"
    names = _record(monkeypatch)
    (x, W, b), dy, r = _linear_case(gpu, rows, 512, N, dt, 12, bias)
    with torch.autocast("cuda", dtype=dt):
        y = proj.linear_splitk(x, W, b)
    y.backward(dy)
    torch.cuda.synchronize()
    assert not [n for n in names if n[1].startswith("dm_gemm")], names
    _linear_verify(case, dt, r, y, x.grad, W.grad, rows, 512, N, dt, bias)
    if bias:                                                       # any order of `rows` fp32 additions of exact 16-bit terms
        _check("b.grad", b.grad, r["db"], rows * EPS32 * r["S_db"])


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_linear_pair_runs_dm_gemm_n_and_equals_linear_splitk(gpu, monkeypatch, dt):
    """linear_pair on two [1, 196, 512] inputs and two [2048, 512] fp32 weights: three dm_gemm launches through the `_n` entry,
    every output and gradient within the bounds and bit for bit that of linear_splitk on that mixer alone."""
    from diffma_amd import projections as proj

    names = _record(monkeypatch)
    cases = [_linear_case(gpu, 196, 512, 2048, dt, 20 + k) for k in (0, 1)]
    (x0, W0, _), dy0, _ = cases[0]
    (x1, W1, _), dy1, _ = cases[1]
    with torch.autocast("cuda", dtype=dt):
        y0, y1 = proj.linear_pair(x0, x1, W0, W1)
    torch.autograd.backward([y0, y1], [dy0, dy1])
    torch.cuda.synchronize()
    assert [n for n in names if n[1] == "dm_gemm"] == [("n", "dm_gemm")] * 3, names
    for k, (y, (x, W, _), dy, r) in enumerate(((y0, *cases[0]), (y1, *cases[1]))):
        _linear_verify(f"pair {k}", dt, r, y, x.grad, W.grad, 196, 512, 2048, F32)
        xs, Ws = x.detach().clone().requires_grad_(True), W.detach().clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dt):
            ys = proj.linear_splitk(xs, Ws)
        ys.backward(dy)
        torch.cuda.synchronize()
        assert torch.equal(ys, y) and torch.equal(xs.grad, x.grad) and torch.equal(Ws.grad, W.grad), k


def test_own_pair_accumulates_in_place_at_the_x_proj_shape(gpu, monkeypatch):
    """du += dx_dbl @ Wx for both mixers in one launch (dx_dbl [2, 588, 64], Wx [2, 64, 1024], du [2, 588, 1024], bf16): per element
    within the accumulate bound."""
    from diffma_amd import projections as proj

    names = _record(monkeypatch)
    g = torch.Generator().manual_seed(31)
    dxd = torch.randn(2, 588, 64, generator=g).to(BF16)
    Wx = (torch.randn(2, 64, 1024, generator=g) * 0.1).to(BF16)
    du0 = torch.randn(2, 588, 1024, generator=g).to(BF16)
    du = du0.to(gpu)
    out = proj._own_pair(dxd.to(gpu), Wx.to(gpu), True, False, du, accumulate=True)
    torch.cuda.synchronize()
    assert names == [("n", "dm_gemm")] and out.data_ptr() == du.data_ptr()
    for k in (0, 1):
        ref, tol, _ = _bound(dxd[k].double() @ Wx[k].double(), dxd[k].double().abs() @ Wx[k].double().abs(), 64, BF16, du0[k].double())
        _check(f"du[{k}]", du[k], ref, tol, key=(BF16, BF16, "own_pair accumulate"))


# =====================================================================================================================================
# 6. K12 (dm_gemm_large) exact on integers
# =====================================================================================================================================
@pytest.mark.parametrize("P,Q,Kc", [(2048, 256, 512), (2163, 512, 1024)], ids=["smallest", "ragged-115-rows"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_gemm_large_exact_on_integers(gpu, dt, P, Q, Kc):
    """The integer construction of section 1 for the persistent large-batch kernel (both operands k-major, C in the operand dtype):
    the smallest shape it takes and one whose last row block has 115 rows; contiguous, with padded rows, and with A the right half
    of a wider buffer and C a column block of a wider sentinel buffer."""
    assert _lib().load().dm_gemm_large_supported(P, Q, Kc, 1, 1, CODE[dt], CODE[dt]) == 1 and P % 256 in (0, 115)
    A, B, _, ref = _int_case(P, Q, Kc)
    Ad, Bd, want = A.to(dt).to(gpu), B.to(dt).to(gpu), ref.to(dt).to(gpu)
    for mode in ("contig", "half"):
        _exact_one(gpu, Ad, Bd, want, 1, 1, mode, entry="dm_gemm_large")
