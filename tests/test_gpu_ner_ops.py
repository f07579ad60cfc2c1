"""The NER kernels of csrc/ner.hip, one op at a time through libner.so's C ABI, against the float64
references and derived bounds of tests/ner_ref.py (whose sensitivity is shown on the CPU by
tests/test_ner_ref.py).  Where the arithmetic allows it the comparison is bit for bit: integer GEMMs
(every partial sum below 2^24, so f32 accumulation is exact in any order and only f2bf's rounding is
left), attention with one kept key, and attention whose softmax is a permutation.

Every output lies between two guard stretches of 0xEE bytes (one row each, rounded up to 16 bytes so
the output stays 16-byte aligned) that must come back untouched; the output itself starts as 0xEE too,
so an element the kernel never wrote cannot pass.  Each comparison prints its worst error-to-bound
ratio (and appends it to the file NER_RATIOS names, if set) before it asserts.

The shapes reach both kernels the default build's ner_gemm can launch (ner_gemm_kernel: k_gemm2 with
128-row tiles up to 16*256 tiles, the single-buffer k_gemm above) and both attention kernels."""
import ctypes
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch

import ner_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

EPS = 1e-12                                  # BertConfig().layer_norm_eps
BF16 = torch.bfloat16
EPIS = (R.EPI_BIAS, R.EPI_GELU, R.EPI_RESID)
GEMM_BIG = (8576, 7936, 64)                  # 67 x 62 = 4154 tiles > 16*256: k_gemm; 4154 % 8 = 2
GEMM_EXACT_SHAPES = [(128, 128, 64), (128, 128, 128), (128, 256, 192), (384, 128, 64), (640, 384, 3072),
                     (1152, 896, 320)]       # 1, 1, 2, 3, 15, 63 tiles; 1, 2, 3, 1, 48, 5 K slabs
GEMM_REAL_SHAPES = [(128, 128, 64), (256, 384, 192), (1024, 2304, 768), (512, 768, 3072)]


@pytest.fixture(scope="module")
def ner():
    lib = pkg("ner").load_library()
    dev = torch.device("cuda", 0)
    return SimpleNamespace(lib=lib, dev=dev, st=lambda: torch.cuda.current_stream(dev).cuda_stream)


def record(comparator, shape, ratio, **extra):
    line = json.dumps(dict(comparator=comparator, shape=shape, ratio=ratio, **extra))
    print("ner_ratio", line)
    if os.environ.get("NER_RATIOS"):
        with open(os.environ["NER_RATIOS"], "a") as f:
            f.write(line + "\n")


class Guarded:
    """rows x cols of dtype on the device between two guard stretches, all bytes 0xEE"""

    def __init__(self, rows, cols, dtype, dev):
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = rows * cols * item
        self.gb = -(-cols * item // 16) * 16
        self.raw = torch.full((2 * self.gb + self.nbytes,), 0xEE, dtype=torch.uint8, device=dev)
        self.out = self.raw[self.gb:self.gb + self.nbytes].view(dtype).view(rows, cols)
        self.ptr = self.out.data_ptr()
        assert self.ptr % 16 == 0

    def guards_intact(self):
        return bool((self.raw[:self.gb] == 0xEE).all()) and bool((self.raw[self.gb + self.nbytes:] == 0xEE).all())

    def untouched(self):
        return bool((self.raw == 0xEE).all())


def dev_bf16(x, dev):
    """a float64 tensor of bf16-representable values as a bf16 device tensor (the cast is exact)"""
    return x.to(BF16).to(dev).contiguous()


def dev_f32(x, dev):
    return x.to(torch.float32).to(dev).contiguous()


def ptr(t):
    return t.data_ptr() if t is not None else None


def run_gemm(ner, dA, dW, dbias, dR, epi):
    M, K = dA.shape
    N = dW.shape[0]
    out = Guarded(M, N, BF16, ner.dev)
    rc = ner.lib.ner_gemm(ptr(dA), ptr(dW), ptr(dbias), ptr(dR), out.ptr, M, N, K, epi, ner.st())
    assert rc == 0
    got = out.out.cpu()
    assert out.guards_intact(), "ner_gemm wrote outside its [M, N] output"
    return got


# ------------------------------------------------------------------------------------------- GEMM
def gemm_ints(M, N, K):
    """integer operands, exact in bf16 / f32: |A|, |W| <= 8, |bias| <= 64, |R| <= 256, so every partial
    sum is an integer of magnitude <= 64 K + 320 < 2^24 (K <= 3072) and the f32 result is exact"""
    assert 64 * K + 320 < 2 ** 24
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float64)     # noqa: E731
    return SimpleNamespace(A=ri(-8, 8, M, K), W=ri(-8, 8, N, K), bias=ri(-64, 64, N),
                           R=torch.randint(-256, 257, (M, N), generator=g, dtype=torch.int16).to(BF16))   # (kept narrow: [M, N])


def gemm_reals(M, N, K, gelu_spread=False):
    """the operands of tests/test_ner.py; gelu_spread: a bias ramp that spreads the pre-activations
    over about [-8, 8], so GELU's negative tail (|gelu(v)| < 0.05 for v < -2) is populated"""
    g = torch.Generator().manual_seed(M + N + K)
    A = R.bf(torch.randn(M, K, generator=g))
    W = R.bf(torch.randn(N, K, generator=g) * 0.05)
    bias = torch.randn(N, generator=g).to(torch.float32).to(torch.float64)
    Rs = torch.randn(M, N, generator=g).to(BF16)               # (kept narrow: [M, N])
    if gelu_spread:
        bias = torch.linspace(-7.5, 7.5, N)[torch.randperm(N, generator=g)].to(torch.float32).to(torch.float64)
    return SimpleNamespace(A=A, W=W, bias=bias, R=Rs)


def to_dev(d, dev):
    return SimpleNamespace(A=dev_bf16(d.A, dev), W=dev_bf16(d.W, dev), bias=dev_f32(d.bias, dev), R=dev_bf16(d.R, dev))


def check_exact(ner, d, dd, epi, with_bias, shape):
    bias, dbias = (d.bias, dd.bias) if with_bias else (None, None)
    got = run_gemm(ner, dd.A, dd.W, dbias, dd.R if epi == R.EPI_RESID else None, epi)
    bad, big = R.gemm_exact(got, d.A, d.W, bias, d.R, epi)
    record("gemm_exact", list(shape), 0.0 if bad == 0 else math.inf, epi=epi, bias=with_bias, mismatches=bad,
           above_256=round(big, 4), kernel=ner.lib.ner_gemm_kernel(shape[0], shape[1]))
    assert big >= 0.05, big                   # bf16 holds every integer only up to 256: rounding and ties occur
    assert bad == 0, (epi, with_bias, bad)


@pytest.mark.parametrize("M,N,K", GEMM_EXACT_SHAPES)
def test_gemm_exact_integers(ner, M, N, K):
    d = gemm_ints(M, N, K)
    dd = to_dev(d, ner.dev)
    for epi in (R.EPI_BIAS, R.EPI_RESID):
        for with_bias in (True, False):
            check_exact(ner, d, dd, epi, with_bias, (M, N, K))


@pytest.fixture(scope="module")
def big_ints(ner):
    d = gemm_ints(*GEMM_BIG)
    return d, to_dev(d, ner.dev)


@pytest.mark.parametrize("epi", EPIS)
def test_gemm_exact_integers_single_buffer_kernel(ner, big_ints, epi):
    """k_gemm (its own epilogue, the XCD remap at 4154 workgroups): exact for bias and residual, GELU of
    the integer pre-activations under its bound"""
    d, dd = big_ints
    assert ner.lib.ner_gemm_kernel(GEMM_BIG[0], GEMM_BIG[1]) == 0
    if epi == R.EPI_GELU:
        got = run_gemm(ner, dd.A, dd.W, dd.bias, None, epi)
        r = R.gemm_ratio(got, d.A, d.W, d.bias, None, epi)
        record("gemm_gelu_integers", list(GEMM_BIG), r, epi=epi, kernel=0)
        assert r <= 1
    else:
        check_exact(ner, d, dd, epi, True, GEMM_BIG)


def test_gemm_null_bias_single_buffer_kernel(ner, big_ints):
    d, dd = big_ints
    check_exact(ner, d, dd, R.EPI_RESID, False, GEMM_BIG)


def test_gemm_kernel_paths_all_reached(ner):
    """ner_gemm_kernel is the predicate ner_gemm dispatches on.  The shapes of this file must reach
    every kernel this build can launch for any shape: a moved threshold or a newly enabled tile size
    then fails here instead of leaving a kernel untested."""
    k = ner.lib.ner_gemm_kernel
    reachable = {k(128 * m, 128 * n) for m in [1, 2, 3, 4, 6, 8, 9, 16, 24, 32, 64, 67, 128, 512, 4096]
                 for n in [1, 2, 3, 6, 7, 18, 24, 62, 64]}
    tested = {k(M, N) for M, N, _ in GEMM_EXACT_SHAPES + GEMM_REAL_SHAPES + [GEMM_BIG]}
    assert reachable <= {0, 1, 2}
    assert tested == reachable, (tested, reachable)
    assert {k(M, N) for M, N, _ in GEMM_EXACT_SHAPES + GEMM_REAL_SHAPES} == {1} and k(*GEMM_BIG[:2]) == 0
    # the tile counts promised above: nwg % 8 != 0 everywhere, so the remap's short XCDs are exercised
    assert [(M // 128) * (N // 128) for M, N, _ in GEMM_EXACT_SHAPES] == [1, 1, 2, 3, 15, 63]
    assert (GEMM_BIG[0] // 128) * (GEMM_BIG[1] // 128) == 4154 > 16 * 256


def check_real(ner, d, dd, epi, shape):
    got = run_gemm(ner, dd.A, dd.W, dd.bias, dd.R if epi == R.EPI_RESID else None, epi)
    r = R.gemm_ratio(got, d.A, d.W, d.bias, d.R, epi)
    record("gemm_real", list(shape), r, epi=epi, kernel=ner.lib.ner_gemm_kernel(shape[0], shape[1]))
    assert r <= 1, (epi, r)


def assert_gelu_spread(d):
    v = R.gemm_ref(d.A[:128], d.W, d.bias, None, R.EPI_GELU)[0]
    assert float(v.min()) < -7 and float(v.max()) > 7
    assert float(((v < -2) & (v > -8)).double().mean()) > 0.2            # the tail an absolute 1e-2 cannot see


@pytest.mark.parametrize("M,N,K", GEMM_REAL_SHAPES)
def test_gemm_real_valued(ner, M, N, K):
    d = gemm_reals(M, N, K)
    dd = to_dev(d, ner.dev)
    for epi in (R.EPI_BIAS, R.EPI_RESID):
        check_real(ner, d, dd, epi, (M, N, K))
    d = gemm_reals(M, N, K, gelu_spread=True)
    assert_gelu_spread(d)
    check_real(ner, d, to_dev(d, ner.dev), R.EPI_GELU, (M, N, K))


@pytest.fixture(scope="module")
def big_reals(ner):
    d = gemm_reals(*GEMM_BIG)
    return d, to_dev(d, ner.dev)


@pytest.mark.parametrize("epi", EPIS)
def test_gemm_real_valued_single_buffer_kernel(ner, big_reals, epi):
    d, dd = big_reals
    if epi == R.EPI_GELU:                            # the same operands under the spread bias
        d = SimpleNamespace(A=d.A, W=d.W, R=None, bias=gemm_reals(128, GEMM_BIG[1], 64, gelu_spread=True).bias)
        dd = SimpleNamespace(A=dd.A, W=dd.W, R=None, bias=dev_f32(d.bias, ner.dev))
        assert_gelu_spread(d)
    check_real(ner, d, dd, epi, GEMM_BIG)


@pytest.mark.parametrize("epi", EPIS)
def test_gemm_inf_and_nan_bias_stay_in_their_columns(ner, epi):
    M, N, K = 256, 384, 192
    d = gemm_reals(M, N, K)
    dd = to_dev(d, ner.dev)
    dR = dd.R if epi == R.EPI_RESID else None
    clean = run_gemm(ner, dd.A, dd.W, dd.bias, dR, epi)
    bias = d.bias.clone()
    ci, cn = 5, 130                                  # in different 8-column chunks and different tiles
    bias[ci], bias[cn] = math.inf, math.nan
    got = run_gemm(ner, dd.A, dd.W, dev_f32(bias, ner.dev), dR, epi)
    assert bool((got[:, ci].float() == math.inf).all())
    assert bool(torch.isnan(got[:, cn].float()).all())
    keep = torch.ones(N, dtype=torch.bool)
    keep[ci] = keep[cn] = False
    assert torch.equal(R.bf16_bits(got)[:, keep], R.bf16_bits(clean)[:, keep])


# -------------------------------------------------------------------------------------- attention
ATT_S_MFMA = [32, 64, 96, 128]
ATT_S_GENERAL = [1, 31, 33, 48, 160, 256]
ATT_B = 3


def run_attention(ner, qkv, mask, B, S, heads):
    out = Guarded(B * S, heads * 64, BF16, ner.dev)
    dq = dev_bf16(qkv, ner.dev)
    dm = mask.to(torch.int32).to(ner.dev).contiguous() if mask is not None else None
    rc = ner.lib.ner_attention(ptr(dq), ptr(dm), out.ptr, B, S, heads, 64, ner.st())
    assert rc == 0
    got = out.out.cpu()
    assert out.guards_intact(), "ner_attention wrote outside its output"
    return got


def attention_masks(S, g):
    """name -> mask [3, S] (None = NULL).  S = 1 makes some of these fully masked sequences, which is
    defined: zeros."""
    B = ATT_B
    ones = lambda: torch.ones(B, S, dtype=torch.int32)                       # noqa: E731
    m = {"none": None}
    x = ones()
    for b, n in enumerate([S, max(1, S * 5 // 8), max(1, S // 3)]):
        x[b, n:] = 0
    m["lengths"] = x
    x = (torch.rand(B, S, generator=g) < 0.7).to(torch.int32)
    x[:, S - 1] = 1
    m["holes"] = x
    x = ones()
    x[:, 0] = 0
    m["first_key"] = x
    x = ones()
    lo, hi = (32, 64) if S >= 64 else (S // 3, max(S // 3 + 1, 2 * S // 3))   # a whole 32-key tile where there is one
    x[:, lo:hi] = 0
    m["tile"] = x
    x = ones()
    x[0, max(1, S // 2):] = 0
    x[1] = 0
    x[2, :S // 4] = 0
    m["one_sequence_masked"] = x
    return m


def att_cases():
    return [(h, S) for h in (3, 12) for S in ATT_S_MFMA + ATT_S_GENERAL]


@pytest.mark.parametrize("heads,S", att_cases())
def test_attention_random_inputs_under_masks(ner, heads, S):
    B = ATT_B
    g = torch.Generator().manual_seed(1000 * heads + S)
    qkv = R.bf(torch.randn(B * S, 3 * heads * 64, generator=g))
    mfma = R.attention_is_mfma(S)
    assert mfma == (S in ATT_S_MFMA)
    for name, mask in attention_masks(S, g).items():
        got = run_attention(ner, qkv, mask, B, S, heads)
        ref, absv = R.attention_ref(qkv, mask, B, S, heads)
        r = R.ratio(got, ref, R.attention_bound(ref, absv, mfma))
        record("attention_mfma" if mfma else "attention_general", [B, S, heads], r, mask=name)
        assert r <= 1, (name, r)
        if name == "one_sequence_masked":
            assert not got[S:2 * S].float().any(), "a sequence with no kept key must come back as zeros"
            assert got[:S].float().any() and got[2 * S:].float().any()


@pytest.mark.parametrize("heads,S", att_cases())
def test_attention_one_kept_key_is_exact(ner, heads, S):
    """softmax over one key is 1: every query row of the sequence is that key's V row, bit for bit"""
    B, H = ATT_B, heads * 64
    g = torch.Generator().manual_seed(2000 * heads + S)
    qkv = R.bf(torch.randn(B * S, 3 * H, generator=g))
    kept = [0, S - 1, S // 2]
    mask = torch.zeros(B, S, dtype=torch.int32)
    for b, j in enumerate(kept):
        mask[b, j] = 1
    got = R.bf16_bits(run_attention(ner, qkv, mask, B, S, heads)).reshape(B, S, H)
    v = R.bf16_bits(qkv[:, 2 * H:]).reshape(B, S, H)
    for b, j in enumerate(kept):
        assert torch.equal(got[b], v[b, j].expand(S, H)), (b, j)


@pytest.mark.parametrize("heads,S", att_cases())
def test_attention_permutation_is_exact(ner, heads, S):
    """K_j = 4 (+-1)^64 and Q_i = K_perm(i): query i scores 128 on key perm(i) and 2 (k_i . k_j) / 16 on the
    others.  With the lead asserted below (>= 40) every other probability is below e^-40 = 4.3e-18, so
    l = 1 and the weighted sum differs from V[perm(i)] by less than S e^-40 max|V| < 1e-14, which is
    below half an f32 ulp of any |V| >= 2^-10: the output is V[perm(i)] bit for bit.  This pins which
    key each P / V^T operand element belongs to, and the i < nkt key tiles."""
    B, H = ATT_B, heads * 64
    g = torch.Generator().manual_seed(3000 * heads + S)
    x = torch.zeros(B, S, 3, heads, 64, dtype=torch.float64)
    k = 4.0 * (torch.randint(0, 2, (B, S, heads, 64), generator=g) * 2 - 1).to(torch.float64)
    perm = torch.stack([torch.randperm(S, generator=g) for _ in range(B)])
    v = R.bf(torch.randn(B, S, heads, 64, generator=g))
    v = torch.where(v.abs() < 2.0 ** -10, torch.full_like(v, 2.0 ** -10), v)
    x[:, :, 0] = torch.stack([k[b, perm[b]] for b in range(B)])
    x[:, :, 1] = k
    x[:, :, 2] = v
    if S > 1:
        sc = torch.einsum("bihd,bjhd->bhij", x[:, :, 0], k) / 8.0
        top2 = sc.topk(2, dim=-1).values
        assert bool((sc.argmax(-1) == perm[:, None, :]).all())
        lead = float((top2[..., 0] - top2[..., 1]).min())
        print("permutation lead", S, heads, lead)
        assert lead >= 40, lead
    got = R.bf16_bits(run_attention(ner, x.reshape(B * S, 3 * H), None, B, S, heads)).reshape(B, S, H)
    vb = R.bf16_bits(v.reshape(B, S, H))
    for b in range(B):
        assert torch.equal(got[b], vb[b, perm[b]]), b


# ------------------------------------------------------------------- LayerNorm, embed, classify
LN_M = [1, 3, 4, 5, 129]                     # row >= M exits in the last workgroup (4 rows each), one full wave
LN_H = [1, 63, 64, 65, 768, 1000, 1024]      # the c < H tail inside and across the 64-lane steps, the limit


def ln_rows(g, M, H):
    """random rows (mean 1, spread 3), a constant row (variance 0: the output is beta) and a row of
    mean 100 and spread about 1 (a variance taken without the mean, or over padded columns, is off by
    orders of magnitude there)"""
    x = torch.randn(M, H, generator=g) * 3 + 1
    if M > 1:
        x[0] = 2.5
    x[M - 1] = 100 + torch.randn(H, generator=g)
    return R.bf(x)


def ln_params(g, H):
    f = lambda: torch.randn(H, generator=g).to(torch.float32).to(torch.float64)   # noqa: E731
    return f(), f()


@pytest.mark.parametrize("H", LN_H)
def test_layernorm(ner, H):
    g = torch.Generator().manual_seed(H)
    gamma, beta = ln_params(g, H)
    dg, db = dev_f32(gamma, ner.dev), dev_f32(beta, ner.dev)
    for M in LN_M:
        x = ln_rows(g, M, H)
        out = Guarded(M, H, BF16, ner.dev)
        dx = dev_bf16(x, ner.dev)
        assert ner.lib.ner_layernorm(ptr(dx), ptr(dg), ptr(db), out.ptr, M, H, EPS, ner.st()) == 0
        got = out.out.cpu()
        assert out.guards_intact()
        ref, xhat = R.layernorm_ref(x, gamma, beta, EPS)
        r = R.ratio(got, ref, R.layernorm_bound(ref, xhat, gamma, beta))
        record("layernorm", [M, H], r)
        assert r <= 1, (M, r)
        if M > 1:
            assert torch.equal(R.bf16_bits(got[0]), R.bf16_bits(R.rne_bf16(beta)))   # variance 0


@pytest.mark.parametrize("H", LN_H)
def test_embed(ner, H):
    g = torch.Generator().manual_seed(100 + H)
    vocab = 50
    gamma, beta = ln_params(g, H)
    dg, db = dev_f32(gamma, ner.dev), dev_f32(beta, ner.dev)
    wemb = R.bf(torch.randn(vocab, H, generator=g))
    temb = R.bf(torch.randn(H, generator=g))
    dw, dt = dev_bf16(wemb, ner.dev), dev_bf16(temb, ner.dev)
    for S in (1, 7, 64):
        # (as many position rows as token rows: an index that forgot the % S reads a wrong row, not past the table)
        pemb = R.bf(torch.randn(max(S, max(LN_M)), H, generator=g))
        dp = dev_bf16(pemb, ner.dev)
        for M in LN_M:
            ids = torch.randint(0, vocab, (M,), generator=g).to(torch.int32)
            ids[0] = vocab - 1
            ids[M - 1] = 0 if M > 1 else vocab - 1
            if M > 2:
                ids[1] = 0
            out = Guarded(M, H, BF16, ner.dev)
            di = ids.to(ner.dev)
            assert ner.lib.ner_embed(ptr(di), ptr(dw), ptr(dp), ptr(dt), ptr(dg), ptr(db), out.ptr, M, S, H, EPS,
                                     ner.st()) == 0
            got = out.out.cpu()
            assert out.guards_intact()
            ref, xhat = R.embed_ref(ids, wemb, pemb, temb, gamma, beta, S, EPS)
            r = R.ratio(got, ref, R.layernorm_bound(ref, xhat, gamma, beta))
            record("embed", [M, S, H], r)
            assert r <= 1, (M, S, r)


@pytest.mark.parametrize("H", LN_H)
def test_classify(ner, H):
    g = torch.Generator().manual_seed(200 + H)
    for L in (1, 3, 9):
        Wc = R.bf(torch.randn(L, H, generator=g) * 0.05)
        bc = torch.randn(L, generator=g).to(torch.float32).to(torch.float64)
        dW, dbc = dev_bf16(Wc, ner.dev), dev_f32(bc, ner.dev)
        for M in LN_M:
            h = R.bf(torch.randn(M, H, generator=g))
            out = Guarded(M, L, torch.float32, ner.dev)
            dh = dev_bf16(h, ner.dev)
            assert ner.lib.ner_classify(ptr(dh), ptr(dW), ptr(dbc), out.ptr, M, H, L, ner.st()) == 0
            got = out.out.cpu()
            assert out.guards_intact()
            ref, bound = R.classify_ref(h, Wc, bc)
            r = R.ratio(got, ref, bound)
            record("classify", [M, H, L], r)
            assert r <= 1, (M, L, r)


# ---------------------------------------------------------------------------------- argument errors
def test_gemm_argument_errors(ner):
    """each returns -1 before anything is launched, so the output stays as it was"""
    dev = ner.dev
    A = torch.zeros(256, 256, dtype=BF16, device=dev)          # large enough for every shape below
    W = torch.zeros(256, 256, dtype=BF16, device=dev)
    bias = torch.zeros(256, dtype=torch.float32, device=dev)
    Rs = torch.zeros(256, 256, dtype=BF16, device=dev)
    out = Guarded(256, 256, BF16, dev)
    ok = (128, 128, 64, R.EPI_BIAS, Rs)
    bad = [(128, 128, 0), (128, 128, -64), (128, 0, 64), (128, -128, 64), (0, 128, 64), (-128, 128, 64),
           (130, 128, 64), (128, 200, 64), (128, 128, 96), (64, 128, 64), (128, 64, 64), (128, 128, 32)]
    calls = [(M, N, K, R.EPI_BIAS, Rs) for M, N, K in bad]
    calls += [ok[:3] + (3, Rs), ok[:3] + (-1, Rs), ok[:3] + (R.EPI_RESID, None)]
    for M, N, K, epi, r in calls:
        rc = ner.lib.ner_gemm(ptr(A), ptr(W), ptr(bias), ptr(r), out.ptr, M, N, K, epi, ner.st())
        assert rc == -1, (M, N, K, epi)
    for null in range(3):                                       # A, W or C missing
        p = [ptr(A), ptr(W), out.ptr]
        p[null] = None
        assert ner.lib.ner_gemm(p[0], p[1], ptr(bias), ptr(Rs), p[2], 128, 128, 64, 0, ner.st()) == -1
    torch.cuda.synchronize(dev)
    assert out.untouched()


def test_attention_argument_errors(ner):
    dev = ner.dev
    qkv = torch.zeros(3 * 257, 3 * 64, dtype=BF16, device=dev)
    out = Guarded(3 * 257, 64, BF16, dev)
    for B, S, heads, dhead in [(1, 0, 1, 64), (1, 257, 1, 64), (1, 64, 1, 32), (1, -32, 1, 64), (0, 64, 1, 64),
                               (1, 64, 0, 64)]:
        assert ner.lib.ner_attention(ptr(qkv), None, out.ptr, B, S, heads, dhead, ner.st()) == -1, (B, S, heads, dhead)
    torch.cuda.synchronize(dev)
    assert out.untouched()


def test_layernorm_embed_classify_argument_errors(ner):
    dev = ner.dev
    x = torch.zeros(4, 1088, dtype=BF16, device=dev)
    vec = torch.zeros(1088, dtype=torch.float32, device=dev)
    ids = torch.zeros(4, dtype=torch.int32, device=dev)
    out = Guarded(4, 1088, BF16, dev)
    logits = Guarded(4, 3, torch.float32, dev)
    for H in (0, 1025, -64):
        assert ner.lib.ner_layernorm(ptr(x), ptr(vec), ptr(vec), out.ptr, 4, H, EPS, ner.st()) == -1, H
        assert ner.lib.ner_embed(ptr(ids), ptr(x), ptr(x), ptr(x), ptr(vec), ptr(vec), out.ptr, 4, 2, H, EPS,
                                 ner.st()) == -1, H
    assert ner.lib.ner_layernorm(ptr(x), ptr(vec), ptr(vec), out.ptr, 0, 64, EPS, ner.st()) == -1
    assert ner.lib.ner_embed(ptr(ids), ptr(x), ptr(x), ptr(x), ptr(vec), ptr(vec), out.ptr, 4, 0, 64, EPS,
                             ner.st()) == -1
    for M, H, L in [(4, 0, 3), (4, -64, 3), (0, 64, 3), (4, 64, 0)]:
        assert ner.lib.ner_classify(ptr(x), ptr(x), ptr(vec), logits.ptr, M, H, L, ner.st()) == -1, (M, H, L)
    torch.cuda.synchronize(dev)
    assert out.untouched() and logits.untouched()


def test_abi_declares_the_path_query(ner):
    assert ner.lib.ner_gemm_kernel.restype is ctypes.c_int and len(ner.lib.ner_gemm_kernel.argtypes) == 2
