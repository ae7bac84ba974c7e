"""vc_gemm / vc_gemm_ex / vc_gemm_group_* / vc_gemm_colstats / vc_colsum(_ex) off their natural layouts, on the
MI355X: every kernel family against a float64 product written here, at the operand layouts on which the host-side
plan (gemm_impl) changes its choice -- leading dimensions above the natural width (aligned and not), base pointers
off 16 B, batch strides that are no multiple of 4 -- with the whole epilogue (alpha < 0, beta outside {0, 1}, bias,
row-modulo addend with add_ld > N, ReLU, the ReLU mask flags & 64, the bias gradient's ones column beside a full tile
column) and workspaces so tight that the split-K clamps act.

Inputs are helpers.Poisoned (lead, gap columns and tail NaN: no kernel may let operand padding reach an output),
outputs and workspaces helpers.Guarded (NaN, or the accumulated-into values; gaps and a 64-element guard must stay
bit-identical).  Bounds: 1e-5 of max |ref| on random data (bf16 kernels: against the product of the RNE-rounded
operands); torch.equal on integer data, where every partial sum is an integer below 2^24 and so exact in any
summation order (exact_case: checked on the CPU, also without a GPU).
"""
import ctypes
import functools

import pytest
import torch

from helpers import Guarded, Poisoned, rel_err, within
from test_kernels_gpu import F_BF16, F_LEGACY, F_NOPIPE, F_PIPE, GROUP_BYTES, KERNELS, bf16_round, rnd

gpu = pytest.mark.gpu
DEV = "cuda"
F_RELU, F_MASK = 1, 64
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
KIDS = [f"k{k}" for k in KERNELS]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vitcnn_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def ws():
    return torch.empty(1 << 22, device=DEV)


@pytest.fixture(scope="module")
def cnt():
    return torch.zeros(1 << 12, dtype=torch.int32, device=DEV)


def S():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return t.data_ptr() if t is not None else None


def up4(n):
    return -(-n // 4) * 4


# operand layouts: name -> (leading dimension of a natural width w, lead elements before the base)
LAYOUTS = {
    "nat": lambda w: (w, 0),
    "pad4": lambda w: (w + 4, 0),        # aligned and padded: the pipelined kernel still fits when w % 4 == 0
    "pad3": lambda w: (w + 3, 0),
    "lead1": lambda w: (up4(w), 1),      # the leading dimension would allow vectors, the base does not
}
# (layout of A, layout of B): the four layouts on both, then mixed pairs (va != vb in the k-major / K-contiguous
# kernels; one operand keeping the pipelined kernel from fitting)
PAIRS = [("nat", "nat"), ("pad4", "pad4"), ("pad3", "pad3"), ("lead1", "lead1"), ("pad4", "pad3"), ("lead1", "pad4"),
         ("nat", "lead1")]


def place(t, layout):
    ld, lead = LAYOUTS[layout](t.shape[-1])
    return Poisoned(t, ld=ld, lead=lead)


def ints(*shape, seed=0, lo=-4, hi=4, even=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, shape, generator=g).float()
    return 2 * torch.div(t, 2, rounding_mode="trunc") if even else t


@functools.lru_cache(maxsize=None)
def operands(ta, tb, M, N, K, exact=False, even_a=False):
    """A as stored ([K, M] if transA else [M, K]) and B as stored ([N, K] if transB else [K, N])"""
    sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    if exact:
        return ints(*sa, seed=101, even=even_a), ints(*sb, seed=102)
    return rnd(*sa, seed=101), rnd(*sb, seed=102)


@functools.lru_cache(maxsize=None)
def product(ta, tb, M, N, K, bf, exact=False, even_a=False):
    """float64 op(A) op(B) of the (bf16-rounded, if bf) operands"""
    A, B = operands(ta, tb, M, N, K, exact, even_a)
    if bf:
        A, B = bf16_round(A), bf16_round(B)
    return (A.t() if ta else A).double() @ (B.t() if tb else B).double()


def epilogue_ref(prod, alpha=1.0, beta=0.0, C0=None, bias=None, addend=None, add_mod=0, flags=0):
    """the header's formula, float64: alpha op(A) op(B) + beta C (+ bias[n]) (+ addend[m % add_mod, n] | mask) (ReLU)"""
    M = prod.shape[-2]
    v = alpha * prod
    if beta != 0.0:
        v = v + beta * C0.double()
    if bias is not None:
        v = v + bias.double()
    if addend is not None:
        a = addend.double()[torch.arange(M) % (add_mod if add_mod > 0 else M)]
        v = torch.where(a > 0, v, torch.zeros((), dtype=torch.float64)) if flags & F_MASK else v + a
    if flags & F_RELU:
        v = torch.relu(v)
    return v


def exact_case(ta, tb, M, N, K, alpha, beta, with_extras, bf=False):
    """Integer operands in [-4, 4] (A even where alpha = 0.5, C0 even where beta = 0.5), integer C0 / bias / addend:
    returns (C0, bias, addend, ref) after asserting that the float64 reference is integer-valued and below 2^24,
    and that so is every partial sum whatever its order (sum_k |a| |b| < 2^24) -- then fp32 (and bf16 operands:
    integers up to 4 are exact) accumulate without rounding and the kernel must return ref bit for bit."""
    even_a = alpha == 0.5
    A, B = operands(ta, tb, M, N, K, True, even_a)
    prod = product(ta, tb, M, N, K, bf, True, even_a)
    C0 = ints(M, N, seed=103, lo=-8, hi=8, even=beta == 0.5) if beta != 0.0 else None
    bias = ints(N, seed=104, lo=-8, hi=8) if with_extras else None
    addend = ints(7, N, seed=105, lo=-8, hi=8) if with_extras else None
    ref = epilogue_ref(prod, alpha, beta, C0, bias, addend, 7 if with_extras else 0)
    worst = float(((A.t() if ta else A).abs().double() @ (B.t() if tb else B).abs().double()).max())
    assert worst < 2 ** 24 and K <= 4100
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2 ** 24
    assert torch.equal(ref.float().double(), ref)
    return C0, bias, addend, ref


def gemm(L, ta, tb, M, N, K, Ap, Bp, kern, C, *, alpha=1.0, beta=0.0, bias=None, addend=None, add_mod=0, flags=0,
         bias_grad=None, ws_ptr=None, ws_n=0, counters=None, group=None, batch=1):
    """one vc_gemm / vc_gemm_ex / vc_gemm_group_add call over placed operands (Poisoned) into C (Guarded)"""
    args = (ta, tb, M, N, K, alpha, Ap.ptr, Ap.ld, Ap.stride if batch > 1 else 0, Bp.ptr, Bp.ld,
            Bp.stride if batch > 1 else 0, beta, C.ptr, C.ld, C.stride if batch > 1 else 0, batch,
            P(bias), addend.ptr if addend is not None else None, addend.ld if addend is not None else 0, add_mod,
            kern | flags, bias_grad.ptr if bias_grad is not None else None, ws_ptr, ws_n)
    if group is not None:
        return L.vc_gemm_group_add(group, *args, P(counters), counters.numel() if counters is not None else 0)
    if counters is not None:
        return L.vc_gemm_ex(*args, P(counters), counters.numel(), S())
    return L.vc_gemm(*args, S())


MATRIX_SHAPES = [(1, 1, 1), (37, 41, 9), (65, 63, 36), (130, 70, 260)]   # the last: split-K on every family with a ws
EXACT_AB = [(1.0, 0.0), (-2.0, 0.5), (0.5, 1.0), (1.0, -2.0), (-2.0, 1.0), (0.5, 0.5), (1.0, 1.0)]   # one per PAIRS entry


# ------------------------------------------------------------------------------------------ a. layout matrix
@gpu
@pytest.mark.parametrize("kern", KERNELS, ids=KIDS)
@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("M,N,K", MATRIX_SHAPES)
def test_layout_matrix(L, ws, kern, ta, tb, M, N, K):
    A, B = operands(ta, tb, M, N, K)
    bias = rnd(N, seed=3)
    ref = epilogue_ref(product(ta, tb, M, N, K, bool(kern & F_BF16)), bias=bias)
    bd = bias.to(DEV)
    for la, lb in PAIRS:
        Ap, Bp = place(A, la), place(B, lb)
        C = Guarded(M, N, ld=N + 5)
        assert gemm(L, ta, tb, M, N, K, Ap, Bp, kern, C, bias=bd, ws_ptr=P(ws), ws_n=ws.numel()) == 0
        within(f"gemm k{kern} t{ta}{tb} {la}/{lb}", f"{M}x{N}x{K}", rel_err(C.check().numpy(), ref.numpy()), 1e-5)


@gpu
@pytest.mark.parametrize("tb", [0, 1])
def test_layout_long_k_automatic_route(L, ws, tb):
    """flags 0, K = 4100 >= 4096 and no transA: the K-contiguous fp32 kernel in slices of <= 2048"""
    M, N, K = 20, 24, 4100
    A, B = operands(0, tb, M, N, K)
    ref = product(0, tb, M, N, K, False)
    for la, lb in PAIRS:
        C = Guarded(M, N, ld=N + 5)
        assert gemm(L, 0, tb, M, N, K, place(A, la), place(B, lb), 0, C, ws_ptr=P(ws), ws_n=ws.numel()) == 0
        within(f"gemm auto t0{tb} {la}/{lb}", f"{M}x{N}x{K}", rel_err(C.check().numpy(), ref.numpy()), 1e-5)


@gpu
@pytest.mark.parametrize("kern", KERNELS, ids=KIDS)
@pytest.mark.parametrize("ta,tb", TRANS)
def test_layout_in_launch_combine(L, cnt, kern, ta, tb):
    """vc_gemm_ex with counters and a workspace of two slabs: every planner splits K in two and the tile's slabs
    (2 x 16 x 32 x 4 B) stay within the in-launch combine's 4096 bytes; the counters are left zero"""
    M, N, K = 16, 32, 512
    A, B = operands(ta, tb, M, N, K)
    ref = product(ta, tb, M, N, K, bool(kern & F_BF16))
    for la, lb in PAIRS:
        C, slabs = Guarded(M, N, ld=N + 5), Guarded(1, 2 * M * N)
        assert gemm(L, ta, tb, M, N, K, place(A, la), place(B, lb), kern, C, ws_ptr=slabs.ptr, ws_n=2 * M * N,
                    counters=cnt) == 0
        within(f"gemm_ex k{kern} t{ta}{tb} {la}/{lb}", f"{M}x{N}x{K}", rel_err(C.check().numpy(), ref.numpy()), 1e-5)
        slabs.check()
        assert int(cnt.abs().sum()) == 0


@gpu
@pytest.mark.parametrize("la,lb", [("nat", "nat"), ("pad3", "lead1")])
def test_layout_bf16_128_row_tile(L, ws, la, lb):
    """F_BF16 | F_NOPIPE at 32 x 32 tiles of 64: the 128-row bf16 tile of the K-contiguous kernel"""
    M, N, K = 2048, 2048, 64
    A, B = operands(0, 1, M, N, K)
    ref = product(0, 1, M, N, K, True)
    C = Guarded(M, N, ld=N + 5)
    assert gemm(L, 0, 1, M, N, K, place(A, la), place(B, lb), F_BF16 | F_NOPIPE, C, ws_ptr=P(ws), ws_n=ws.numel()) == 0
    within(f"gemm bf16 128-row {la}/{lb}", f"{M}x{N}x{K}", rel_err(C.check().numpy(), ref.numpy()), 1e-5)


# ------------------------------------------------------------------------------------------ b. exact cases
def test_exact_generators_are_exact():
    """no GPU: the integer cases' references are integers below 2^24, as is every partial sum"""
    for M, N, K in MATRIX_SHAPES + [(20, 24, 4100)]:
        for ta, tb in TRANS:
            for alpha, beta in EXACT_AB:
                exact_case(ta, tb, M, N, K, alpha, beta, True)


@gpu
@pytest.mark.parametrize("kern", KERNELS, ids=KIDS)
@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("M,N,K", MATRIX_SHAPES)
def test_exact_matrix(L, ws, kern, ta, tb, M, N, K):
    """integer data: a dropped, duplicated or misplaced k element, bias or addend row cannot hide in a tolerance.
    Not the full cross of layouts and scalings: layout pair i runs with the i-th (alpha, beta) of EXACT_AB only
    (every layout pair and every scaling occur, on every selector, transpose and shape; e.g. beta = 0.5 never meets
    the (nat, lead1) pair), which keeps the case at seven launches."""
    for (la, lb), (alpha, beta) in zip(PAIRS, EXACT_AB):
        C0, bias, addend, ref = exact_case(ta, tb, M, N, K, alpha, beta, True, bool(kern & F_BF16))
        A, B = operands(ta, tb, M, N, K, True, alpha == 0.5)
        C = Guarded(M, N, ld=N + 5, init=C0)
        assert gemm(L, ta, tb, M, N, K, place(A, la), place(B, lb), kern, C, alpha=alpha, beta=beta, bias=bias.to(DEV),
                    addend=Poisoned(addend, ld=N + 3), add_mod=7, ws_ptr=P(ws), ws_n=ws.numel()) == 0
        got = C.check()
        assert torch.equal(got.double(), ref), (la, lb, alpha, beta, float((got.double() - ref).abs().max()))


# ------------------------------------------------------------------------------------------ c. epilogue
@gpu
@pytest.mark.parametrize("kern", KERNELS, ids=KIDS)
@pytest.mark.parametrize("M,N,K", [(65, 63, 36), (130, 70, 260)])
def test_epilogue(L, ws, kern, M, N, K):
    """alpha < 0 and beta = 0.5 into a given C0, bias, an addend whose row modulo (7) does not divide M and whose
    leading dimension is N + 3, with and without ReLU; then the ReLU mask (flags | 64) over a layer output holding
    positive, negative, +0.0 and -0.0 entries, with beta = 0.5 and a bias: a masked element is exactly +0, not
    beta C0.  (130, 70, 260) splits K: the epilogue then runs in the combine."""
    bf = bool(kern & F_BF16)
    C0, bias, add7 = rnd(M, N, seed=6, scale=2.0) + 3.0, rnd(N, seed=7), rnd(7, N, seed=8)
    layer = rnd(M, N, seed=9)
    layer.view(-1)[0::5] = 0.0
    layer.view(-1)[1::5] = -0.0
    bd = bias.to(DEV)
    for ta, tb in TRANS:
        A, B = operands(ta, tb, M, N, K)
        prod = product(ta, tb, M, N, K, bf)
        Ap, Bp = place(A, "pad4"), place(B, "pad4")
        for flags in (0, F_RELU):
            ref = epilogue_ref(prod, -0.75, 0.5, C0, bias, add7, 7, flags)
            C = Guarded(M, N, ld=N + 5, init=C0)
            assert gemm(L, ta, tb, M, N, K, Ap, Bp, kern, C, alpha=-0.75, beta=0.5, bias=bd,
                        addend=Poisoned(add7, ld=N + 3), add_mod=7, flags=flags, ws_ptr=P(ws), ws_n=ws.numel()) == 0
            got = C.check()
            within(f"gemm epilogue k{kern} t{ta}{tb} relu={flags}", f"{M}x{N}x{K}", rel_err(got.numpy(), ref.numpy()),
                   1e-5)
            assert not flags or (bool((got == 0).any()) and bool((got > 0).any()))
        ref = epilogue_ref(prod, -0.75, 0.5, C0, bias, layer, 0, F_MASK)
        C = Guarded(M, N, ld=N + 5, init=C0)
        assert gemm(L, ta, tb, M, N, K, Ap, Bp, kern, C, alpha=-0.75, beta=0.5, bias=bd, addend=Poisoned(layer, ld=N + 3),
                    add_mod=0, flags=F_MASK, ws_ptr=P(ws), ws_n=ws.numel()) == 0
        got = C.check()
        within(f"gemm mask k{kern} t{ta}{tb}", f"{M}x{N}x{K}", rel_err(got.numpy(), ref.numpy()), 1e-5)
        dead = ~(layer > 0)
        assert bool(dead.any()) and bool((layer == 0).any()) and bool((layer < 0).any())
        assert bool((got[dead].view(torch.int32) == 0).all())     # +0.0 bit for bit
        assert bool((got[~dead] != 0).all())


@gpu
@pytest.mark.parametrize("kern", KERNELS, ids=KIDS)
@pytest.mark.parametrize("N", [63, 64, 65])
@pytest.mark.parametrize("M,K,split", [(65, 36, False), (130, 260, False), (130, 260, True)])
def test_bias_grad(L, ws, kern, N, M, K, split):
    """the implicit ones column Ne = N + 1 (at N = 64 a tile column of its own) into a guarded [M] vector, beta 0
    and 0.5, with and without split-K; operands aligned and padded so that F_PIPE does take the pipelined kernel"""
    bf = bool(kern & F_BF16)
    A, B = operands(1, 0, M, N, K)
    Ar = bf16_round(A) if bf else A
    prod = product(1, 0, M, N, K, bf)
    Ap, Bp = Poisoned(A, ld=up4(M) + 4), Poisoned(B, ld=up4(N) + 4)
    C0, g0 = rnd(M, N, seed=16), rnd(M, seed=17)
    for beta in (0.0, 0.5):
        C = Guarded(M, N, ld=N + 5, init=C0 if beta else None)
        bg = Guarded(1, M, init=g0 if beta else None)
        assert gemm(L, 1, 0, M, N, K, Ap, Bp, kern, C, alpha=-0.75, beta=beta, bias_grad=bg,
                    ws_ptr=P(ws) if split else None, ws_n=ws.numel() if split else 0) == 0
        shape = f"{M}x{N}x{K} beta={beta} split={int(split)}"
        within(f"gemm+bias_grad C k{kern}", shape,
               rel_err(C.check().numpy(), epilogue_ref(prod, -0.75, beta, C0).numpy()), 1e-5)
        ref_g = -0.75 * Ar.double().sum(0) + beta * g0.double()
        within(f"gemm+bias_grad g k{kern}", shape, rel_err(bg.check()[0].numpy(), ref_g.numpy()), 1e-5)


@gpu
@pytest.mark.parametrize("flags", [F_PIPE, F_BF16 | F_PIPE])
@pytest.mark.parametrize("ta", [0, 1])
def test_bias_grad_transB_declined_by_pipe(L, ws, flags, ta):
    """bias_grad with transB = 1: the pipelined kernel has no ones column there and must decline (pipe_fits);
    the kernel that takes the problem instead still gives the right C and bias gradient"""
    M, N, K = 72, 64, 260
    A, B = operands(ta, 1, M, N, K)
    Ar = bf16_round(A) if flags & F_BF16 else A
    C, bg = Guarded(M, N, ld=N + 5), Guarded(1, M)
    assert gemm(L, ta, 1, M, N, K, place(A, "pad4"), place(B, "pad4"), flags, C, bias_grad=bg, ws_ptr=P(ws),
                ws_n=ws.numel()) == 0
    within(f"gemm transB bias_grad C k{flags} t{ta}1", f"{M}x{N}x{K}",
           rel_err(C.check().numpy(), product(ta, 1, M, N, K, bool(flags & F_BF16)).numpy()), 1e-5)
    ref_g = (Ar.t() if ta else Ar).double().sum(1)
    within(f"gemm transB bias_grad g k{flags} t{ta}1", f"{M}x{N}x{K}", rel_err(bg.check()[0].numpy(), ref_g.numpy()), 1e-5)


# ------------------------------------------------------------------------------------------ d. batched
@gpu
@pytest.mark.parametrize("kern", KERNELS, ids=KIDS)
@pytest.mark.parametrize("M,N,K", [(37, 41, 9), (65, 63, 36)])
def test_batched_odd_strides(L, ws, kern, M, N, K):
    """batch 3 with ReLU: strideA = M lda + 1 (odd: the vector staging must switch off although base and leading
    dimension allow it), strideC = M ldc + 7 with the elements between the batches guarded; then the row-modulo
    addend (a positional embedding over 4 sequences) over a strided A"""
    rd = bf16_round if kern & F_BF16 else (lambda t: t)
    A, B = rnd(3, M, K, seed=21), rnd(3, K, N, seed=22)
    lda, ldc = up4(K), N + 5
    Ap, Bp = Poisoned(A, ld=lda, stride=M * lda + 1), Poisoned(B, ld=up4(N), stride=K * up4(N) + 4)
    C = Guarded(M, N, ld=ldc, batch=3, stride=M * ldc + 7)
    assert gemm(L, 0, 0, M, N, K, Ap, Bp, kern, C, alpha=0.5, flags=F_RELU, batch=3, ws_ptr=P(ws), ws_n=ws.numel()) == 0
    ref = torch.relu(0.5 * torch.bmm(rd(A).double(), rd(B).double()))
    within(f"gemm batched k{kern}", f"3x{M}x{N}x{K}", rel_err(C.check().numpy(), ref.numpy()), 1e-5)
    rows = 4 * M
    A2, W, add = rnd(rows, K, seed=23), rnd(N, K, seed=24), rnd(M, N, seed=25)
    C2 = Guarded(rows, N, ld=ldc)
    assert gemm(L, 0, 1, rows, N, K, Poisoned(A2, ld=K + 3), Poisoned(W, ld=K + 4, lead=1), kern, C2,
                addend=Poisoned(add, ld=N + 3), add_mod=M, ws_ptr=P(ws), ws_n=ws.numel()) == 0
    ref2 = rd(A2).double() @ rd(W).double().t() + add.repeat(4, 1).double()
    within(f"gemm row-modulo addend k{kern}", f"{rows}x{N}x{K}", rel_err(C2.check().numpy(), ref2.numpy()), 1e-5)


# ------------------------------------------------------------------------------------------ e. workspace
SPLIT_CASES = [(k, 0, 1, 130, 70, 260) for k in KERNELS] + [(k, 1, 0, 130, 70, 260) for k in KERNELS] + \
              [(0, 0, 1, 20, 24, 4100), (0, 0, 0, 20, 24, 4100)] + [(k, 0, 1, 16, 32, 512) for k in KERNELS]


@gpu
@pytest.mark.parametrize("kern,ta,tb,M,N,K", SPLIT_CASES)
def test_tight_workspace(L, ws, kern, ta, tb, M, N, K):
    """a workspace of 2 M Ne + 5 floats (the `--nsplit` clamps act), then of M Ne - 1 (no split possible): the
    slabs stay inside it (its guard is untouched, its NaN never reaches C) and the result meets the same bound as
    with the large workspace; with the weight-gradient layout the bias gradient rides along (Ne = N + 1)"""
    ref = product(ta, tb, M, N, K, bool(kern & F_BF16))
    A, B = operands(ta, tb, M, N, K)
    with_bg = bool(ta and not tb)
    Ne = N + int(with_bg)
    Ar = bf16_round(A) if kern & F_BF16 else A
    for n in (None, 2 * M * Ne + 5, M * Ne - 1):
        C, bg = Guarded(M, N, ld=N + 5), (Guarded(1, M) if with_bg else None)
        tight = Guarded(1, n) if n else None
        assert gemm(L, ta, tb, M, N, K, place(A, "nat"), place(B, "pad4"), kern, C, bias_grad=bg,
                    ws_ptr=tight.ptr if n else P(ws), ws_n=n if n else ws.numel()) == 0
        within(f"gemm ws={n} k{kern} t{ta}{tb}", f"{M}x{N}x{K}", rel_err(C.check().numpy(), ref.numpy()), 1e-5)
        if with_bg:
            within(f"gemm ws={n} bias_grad k{kern}", f"{M}x{N}x{K}",
                   rel_err(bg.check()[0].numpy(), Ar.double().sum(0).numpy()), 1e-5)
        if n:
            tight.check()


# ------------------------------------------------------------------------------------------ f. group
GROUP = [
    # ta, tb, M, N, K, layout A, layout B, flags, beta, bias_grad
    (0, 1, 130, 70, 260, "pad4", "pad4", 0, 0.0, False),      # automatic: the pipelined kernel, K split
    (1, 0, 130, 70, 260, "pad3", "nat", 0, 0.0, True),        # k-major, K split, Ne = N + 1
    (0, 0, 65, 63, 36, "lead1", "lead1", F_LEGACY, 1.0, False),
    (1, 1, 37, 41, 9, "pad3", "pad4", 0, 0.0, False),
    (0, 1, 130, 70, 260, "lead1", "pad3", F_LEGACY, 0.5, False),
]


@gpu
def test_group_with_tight_workspace_is_bit_identical(L, cnt):
    """five strided / misaligned problems through vc_gemm_group_*, over a workspace of 2 x 130 x 71 + 5 floats: one
    split problem's slabs fill it, so the group must flush (group_flush) before each next one; results bit-identical
    to the same problems launched alone with the same workspace and counters, guard untouched, counters zero"""
    n = 2 * 130 * 71 + 5
    ins = [(place(operands(ta, tb, M, N, K)[0], la), place(operands(ta, tb, M, N, K)[1], lb))
           for ta, tb, M, N, K, la, lb, _, _, _ in GROUP]
    grp = ctypes.create_string_buffer(GROUP_BYTES)
    outs = []
    for grouped in (False, True):
        tight = Guarded(1, n)
        res = []
        if grouped:
            assert L.vc_gemm_group_begin(ctypes.addressof(grp), S()) == 0
        for i, (ta, tb, M, N, K, _, _, flags, beta, with_bg) in enumerate(GROUP):
            C = Guarded(M, N, ld=N + 5, init=rnd(M, N, seed=40 + i))
            bg = Guarded(1, M) if with_bg else None
            assert gemm(L, ta, tb, M, N, K, ins[i][0], ins[i][1], flags, C, beta=beta, bias_grad=bg, ws_ptr=tight.ptr,
                        ws_n=n, counters=cnt, group=ctypes.addressof(grp) if grouped else None) == 0
            res.append((C, bg))
        if grouped:
            assert L.vc_gemm_group_end(ctypes.addressof(grp)) == 0
        outs.append([(C.check(), bg.check() if bg is not None else None) for C, bg in res])
        tight.check()
        assert int(cnt.abs().sum()) == 0
    for i, ((c0, b0), (c1, b1)) in enumerate(zip(*outs)):
        ta, tb, M, N, K, _, _, _, beta, _ = GROUP[i]
        assert torch.equal(c0, c1), i
        assert b0 is None or torch.equal(b0, b1), i
        ref = epilogue_ref(product(ta, tb, M, N, K, False), 1.0, beta, rnd(M, N, seed=40 + i))
        within(f"gemm group problem {i}", f"{M}x{N}x{K}", rel_err(c1.numpy(), ref.numpy()), 1e-5)


# ------------------------------------------------------------------------------------------ g. colstats
@gpu
@pytest.mark.parametrize("bf", [0, F_BF16])
@pytest.mark.parametrize("M,N,K", [(37, 20, 12), (65, 64, 36), (129, 65, 68)])
def test_colstats_and_bn_apply_partials(L, M, N, K, bf):
    """vc_gemm_colstats (lda = K + 4, ldc = N + 3, the fp64 partials guarded) + vc_bn_apply_partials against the
    float64 train-mode BatchNorm + ReLU of the float64 product, running statistics included"""
    rd = bf16_round if bf else (lambda t: t)
    A, W = rnd(M, K, seed=71) + 0.3, rnd(N, K, seed=72)
    bias, g, bb = rnd(N, seed=73) + 2.0, rnd(N, seed=74) + 1.0, rnd(N, seed=75)
    rm0, rv0 = rnd(N, seed=76), rnd(N, seed=77).abs() + 0.5
    Pn = -(-M // 64)
    pre, cs = Guarded(M, N, ld=N + 3), Guarded(2 * Pn, N, dtype=torch.float64)
    bd, gd, bbd = bias.to(DEV), g.to(DEV), bb.to(DEV)
    Ap, Wp = Poisoned(A, ld=K + 4), Poisoned(W)    # named: the buffers live until the results are read
    assert L.vc_gemm_colstats(M, N, K, Ap.ptr, K + 4, Wp.ptr, K, P(bd), pre.ptr, N + 3, bf, cs.ptr, S()) == 0
    x = rd(A).double() @ rd(W).double().t() + bias.double()
    shape = f"{M}x{N}x{K} bf={bf}"
    within("gemm_colstats C", shape, rel_err(pre.check().numpy(), x.numpy()), 1e-5)
    cs.check()
    mean, inv, rm, rv = Guarded(1, N), Guarded(1, N), Guarded(1, N, init=rm0), Guarded(1, N, init=rv0)
    y = Guarded(M, N, ld=N + 5)
    assert L.vc_bn_apply_partials(M, N, pre.ptr, N + 3, Pn, cs.ptr, P(bd), 1e-5, 0.1, mean.ptr, inv.ptr, rm.ptr, rv.ptr,
                                  P(gd), P(bbd), 1, y.ptr, N + 5, S()) == 0
    rm64, rv64 = rm0.double(), rv0.double()
    ref_y = torch.relu(torch.nn.functional.batch_norm(x, rm64, rv64, g.double(), bb.double(), True, 0.1, 1e-5))
    within("bn_apply_partials y", shape, rel_err(y.check().numpy(), ref_y.numpy()), 1e-5)
    within("bn_apply_partials mean", shape, rel_err(mean.check()[0].numpy(), x.mean(0).numpy()), 1e-5)
    within("bn_apply_partials invstd", shape,
           rel_err(inv.check()[0].numpy(), (1 / torch.sqrt(x.var(0, unbiased=False) + 1e-5)).numpy()), 1e-5)
    within("bn_apply_partials running_mean", shape, rel_err(rm.check()[0].numpy(), rm64.numpy()), 1e-5)
    within("bn_apply_partials running_var", shape, rel_err(rv.check()[0].numpy(), rv64.numpy()), 1e-5)


# ------------------------------------------------------------------------------------------ h. colsum
@gpu
@pytest.mark.parametrize("R", [1, 300, 5000])
@pytest.mark.parametrize("C", [1, 63, 64, 65])
def test_colsum_strided(L, ws, cnt, R, C):
    X, o0 = rnd(R, C, seed=R + C), rnd(C, seed=5)
    Xp = Poisoned(X, ld=C + 3)
    ref = 0.5 * o0.double() + X.double().sum(0)
    outs = []
    for ex in (False, True, True):
        out = Guarded(1, C, init=o0)
        if ex:
            assert L.vc_colsum_ex(R, C, Xp.ptr, C + 3, out.ptr, 0.5, P(ws), ws.numel(), P(cnt), cnt.numel(), S()) == 0
        else:
            assert L.vc_colsum(R, C, Xp.ptr, C + 3, out.ptr, 0.5, P(ws), ws.numel(), S()) == 0
        outs.append(out.check()[0])
        assert int(cnt.abs().sum()) == 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    within("colsum", f"R={R},C={C}", rel_err(outs[0].numpy(), ref.numpy()), 1e-5)
