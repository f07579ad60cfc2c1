"""tests/ner_ref.py on the CPU: each derived bound passes the correctly rounded reference (ratio <= 1)
and fails the rounded result of a subtly wrong computation (ratio > 1) -- the mistakes a kernel of
csrc/ner.hip could make without a loose tolerance noticing.  This is what shows, without a GPU, that
tests/test_gpu_ner_ops.py can fail a wrong kernel without failing a right one."""
import math

import pytest
import torch

import ner_ref as R

EPS = 1e-12


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64)


# ------------------------------------------------------------------------------------------ helpers
def test_rne_bf16_matches_the_format():
    g = _gen(1)
    x = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 8)
    assert torch.equal(R.rne_bf16(x), x.to(torch.bfloat16).to(torch.float64))
    assert torch.equal(R.bf16_bits(R.rne_bf16(x)), R.bf16_bits(x.to(torch.bfloat16)))
    # ties go to the even significand, in both directions; halfway cases of float64, not of f32
    t = torch.tensor([257.0, 259.0, -257.0, -259.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40,
                      0.0, 2.0 ** -133 * 0.5, 2.0 ** -133 * 1.5, 3.3895313892515355e38, 3.4e38, math.inf, -math.inf],
                     dtype=torch.float64)
    want = torch.tensor([256.0, 260.0, -256.0, -260.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7,
                         0.0, 0.0, 2.0 ** -132, 3.3895313892515355e38, math.inf, math.inf, -math.inf], dtype=torch.float64)
    assert torch.equal(R.rne_bf16(t), want)
    assert math.isnan(float(R.rne_bf16(torch.tensor(math.nan))))
    assert R.bf16_bits(torch.tensor([1.0, -2.0, 256.0])).tolist() == [0x3F80, 0xC000, 0x4380]
    with pytest.raises(ValueError):
        R.bf16_bits(torch.tensor([257.0]))
    u = R.ulp_bf16(torch.tensor([1.0, 0.99, 256.0, -300.0, 0.0, 2.0 ** -126, 2.0 ** -130, math.inf]))
    assert u.tolist() == [2.0 ** -7, 2.0 ** -8, 2.0, 2.0, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133, math.inf]
    assert torch.equal(R.trunc_bf16(torch.tensor([259.0, -259.0, 1.99])), torch.tensor([258.0, -258.0, 1.984375],
                                                                                      dtype=torch.float64))


def test_ratio_handles_non_finite_values():
    ref = torch.tensor([1.0, math.inf, math.nan])
    one = torch.ones(3)
    assert R.ratio(torch.tensor([1.5, math.inf, math.nan]), ref, one) == 0.5
    assert R.ratio(torch.tensor([1.0, -math.inf, math.nan]), ref, one) == math.inf
    assert R.ratio(torch.tensor([1.0, math.inf, 0.0]), ref, one) == math.inf
    assert R.ratio(torch.tensor([math.nan, math.inf, math.nan]), ref, one) == math.inf


# --------------------------------------------------------------------------------------------- GEMM
@pytest.fixture(scope="module")
def gemm_int():
    g = _gen(2)
    M, N, K = 128, 128, 192
    return dict(A=_ints(g, -8, 8, M, K), W=_ints(g, -8, 8, N, K), bias=_ints(g, -64, 64, N), R=_ints(g, -256, 256, M, N))


@pytest.fixture(scope="module")
def gemm_real():
    g = _gen(3)
    M, N, K = 128, 128, 192
    return dict(A=R.bf(torch.randn(M, K, generator=g)), W=R.bf(torch.randn(N, K, generator=g) * 0.05),
                bias=torch.randn(N, generator=g).to(torch.float64), R=R.bf(torch.randn(M, N, generator=g)))


def _drop_slab(A):
    A = A.clone()
    A[:, 64:128] = 0
    return A


def _swap_chunks(A):
    """two 16-byte chunks (8 bf16 each) of one row exchanged: a swizzle slip on a single LDS row"""
    A = A.clone()
    A[37, 8:16], A[37, 40:48] = A[37, 40:48].clone(), A[37, 8:16].clone()
    return A


@pytest.mark.parametrize("epi", [R.EPI_BIAS, R.EPI_RESID])
def test_gemm_exact_comparator(gemm_int, epi):
    d = gemm_int
    _, ref = R.gemm_ref(d["A"], d["W"], d["bias"], d["R"], epi)
    bad, big = R.gemm_exact(R.rne_bf16(ref), d["A"], d["W"], d["bias"], d["R"], epi)
    assert bad == 0 and big >= 0.05, (bad, big)             # rounding (and its ties) is exercised
    assert R.gemm_ratio(R.rne_bf16(ref), d["A"], d["W"], d["bias"], d["R"], epi) <= 1
    for wrong_A in (_drop_slab(d["A"]), _swap_chunks(d["A"])):
        _, wrong = R.gemm_ref(wrong_A, d["W"], d["bias"], d["R"], epi)
        assert R.gemm_exact(R.rne_bf16(wrong), d["A"], d["W"], d["bias"], d["R"], epi)[0] > 0
        assert R.gemm_ratio(R.rne_bf16(wrong), d["A"], d["W"], d["bias"], d["R"], epi) > 1
    # truncation stays inside one ulp, so only the exact comparison can see it
    assert R.gemm_exact(R.trunc_bf16(ref), d["A"], d["W"], d["bias"], d["R"], epi)[0] > 0
    # a missing bias (the bias = NULL form confused with the biased one)
    _, nob = R.gemm_ref(d["A"], d["W"], None, d["R"], epi)
    assert R.gemm_exact(R.rne_bf16(nob), d["A"], d["W"], d["bias"], d["R"], epi)[0] > 0
    assert R.gemm_exact(R.rne_bf16(nob), d["A"], d["W"], None, d["R"], epi)[0] == 0


@pytest.mark.parametrize("epi", [R.EPI_BIAS, R.EPI_GELU, R.EPI_RESID])
def test_gemm_bound_comparator(gemm_real, epi):
    d = gemm_real
    _, ref = R.gemm_ref(d["A"], d["W"], d["bias"], d["R"], epi)
    assert R.gemm_ratio(R.rne_bf16(ref), d["A"], d["W"], d["bias"], d["R"], epi, rows=48) <= 1   # (ragged chunks)
    for wrong_A in (_drop_slab(d["A"]), _swap_chunks(d["A"])):
        _, wrong = R.gemm_ref(wrong_A, d["W"], d["bias"], d["R"], epi)
        assert R.gemm_ratio(R.rne_bf16(wrong), d["A"], d["W"], d["bias"], d["R"], epi) > 1


def test_gelu_bound_rejects_tanh_gelu_and_a_flat_negative_tail():
    g = _gen(4)
    M, N, K = 128, 128, 64
    A = R.bf(torch.randn(M, K, generator=g))
    W = R.bf(torch.randn(N, K, generator=g) * 0.125)
    bias = torch.linspace(-7, 7, N, dtype=torch.float64)           # pre-activations over about [-8, 8]
    v, ref = R.gemm_ref(A, W, bias, None, R.EPI_GELU)
    assert float(v.min()) < -7 and float(v.max()) > 7
    assert R.gemm_ratio(R.rne_bf16(ref), A, W, bias, None, R.EPI_GELU) <= 1
    assert R.gemm_ratio(R.rne_bf16(R.gelu_tanh(v)), A, W, bias, None, R.EPI_GELU) > 1
    # zero for every v < -2: invisible to an absolute tolerance of 1e-2
    flat = torch.where(v < -2, torch.zeros_like(ref), ref)
    assert float((flat - ref).abs().max()) < 0.05
    assert R.gemm_ratio(R.rne_bf16(flat), A, W, bias, None, R.EPI_GELU) > 1


# ---------------------------------------------------------------------------------------- attention
@pytest.fixture(scope="module")
def att128():
    g = _gen(5)
    B, S, heads = 3, 128, 3
    qkv = R.bf(torch.randn(B * S, 3 * heads * 64, generator=g))
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[1, 100:] = 0
    mask[2, 17] = 0
    return B, S, heads, qkv, mask


def _att_ratios(got, ref, absv):
    return [R.ratio(got, ref, R.attention_bound(ref, absv, mfma)) for mfma in (True, False)]


def test_attention_bounds_pass_the_rounded_reference(att128):
    B, S, heads, qkv, mask = att128
    for m in (mask, None):
        ref, absv = R.attention_ref(qkv, m, B, S, heads)
        assert max(_att_ratios(R.rne_bf16(ref), ref, absv)) <= 1
    # no kept key: zeros, and only zeros pass
    none = mask.clone()
    none[0] = 0
    ref, absv = R.attention_ref(qkv, none, B, S, heads)
    assert not ref[:S].any() and not absv[:S].any() and ref[S:].any()
    assert max(_att_ratios(R.rne_bf16(ref), ref, absv)) <= 1
    got = R.rne_bf16(ref)
    got[5, 7] = 2.0 ** -120
    assert min(_att_ratios(got, ref, absv)) > 1


def test_attention_bounds_reject_key_mistakes(att128):
    B, S, heads, qkv, mask = att128
    H = heads * 64
    ref, absv = R.attention_ref(qkv, mask, B, S, heads)

    def fails(wrong_qkv, wrong_mask):
        wrong, _ = R.attention_ref(wrong_qkv, wrong_mask, B, S, heads)
        return min(_att_ratios(R.rne_bf16(wrong), ref, absv)) > 1          # the looser (MFMA) bound included

    dropped = mask.clone()
    dropped[0, 77] = 0
    assert fails(qkv, dropped)                                              # one key of 128 dropped
    swapped = qkv.clone()
    r0, r1 = 0 * S + 41, 0 * S + 45                                         # two keys' V rows, one head
    swapped[r0, 2 * H + 64:2 * H + 128], swapped[r1, 2 * H + 64:2 * H + 128] = \
        qkv[r1, 2 * H + 64:2 * H + 128].clone(), qkv[r0, 2 * H + 64:2 * H + 128].clone()
    assert fails(swapped, mask)
    assert fails(qkv, None)                                                 # the mask ignored
    single = mask.clone()
    single[2, 17] = 1                                                       # one masked key let through
    assert fails(qkv, single)


# ------------------------------------------------------------------------- LayerNorm, embed, classify
def _ln_rows(g, M, H):
    x = torch.randn(M, H, generator=g) * 3 + 1
    x[0] = 2.5                                                      # constant row: variance 0
    x[1 % M] = 100 + torch.randn(H, generator=g)                    # mean 100, spread about 1
    return R.bf(x)


def test_layernorm_bound_and_the_padded_variance():
    g = _gen(6)
    M, H = 5, 1000
    x = _ln_rows(g, M, H)
    gamma, beta = torch.randn(H, generator=g).double(), torch.randn(H, generator=g).double()
    ref, xhat = R.layernorm_ref(x, gamma, beta, EPS)
    bound = R.layernorm_bound(ref, xhat, gamma, beta)
    assert R.ratio(R.rne_bf16(ref), ref, bound) <= 1
    assert torch.equal(ref[0], beta)                                # variance 0: exactly beta
    # variance over 1024 columns: the 24 columns past H enter as (0 - mean)^2
    mean = x.mean(-1, keepdim=True)
    var = (((x - mean) ** 2).sum(-1, keepdim=True) + 24 * mean ** 2) / H
    wrong = (x - mean) / torch.sqrt(var + EPS) * gamma + beta
    assert R.ratio(R.rne_bf16(wrong), ref, bound) > 1
    # and the mean over 1024 columns
    mean2 = x.sum(-1, keepdim=True) / 1024
    var2 = ((x - mean2) ** 2).mean(-1, keepdim=True)
    wrong2 = (x - mean2) / torch.sqrt(var2 + EPS) * gamma + beta
    assert R.ratio(R.rne_bf16(wrong2), ref, bound) > 1


def test_embed_bound_and_the_position_index():
    g = _gen(7)
    M, S, H, vocab = 21, 7, 65, 50
    wemb = R.bf(torch.randn(vocab, H, generator=g))
    pemb = R.bf(torch.randn(M, H, generator=g))                     # rows past S exist, as in the model's table
    temb = R.bf(torch.randn(H, generator=g))
    gamma, beta = torch.randn(H, generator=g).double(), torch.randn(H, generator=g).double()
    ids = torch.randint(0, vocab, (M,), generator=g)
    ref, xhat = R.embed_ref(ids, wemb, pemb, temb, gamma, beta, S, EPS)
    bound = R.layernorm_bound(ref, xhat, gamma, beta)
    assert R.ratio(R.rne_bf16(ref), ref, bound) <= 1
    wrong, _ = R.embed_ref(ids, wemb, pemb, temb, gamma, beta, M, EPS)      # pos = row, not row % S
    assert torch.equal(wrong[:S], ref[:S])
    assert R.ratio(R.rne_bf16(wrong), ref, bound) > 1
    wrong, _ = R.layernorm_ref(R.embed_sum(ids, wemb, pemb, temb, S) - R.f64(temb), gamma, beta, EPS)   # type row lost
    assert R.ratio(R.rne_bf16(wrong), ref, bound) > 1


def test_classify_bound():
    g = _gen(8)
    M, H, L = 5, 1000, 3
    h = R.bf(torch.randn(M, H, generator=g))
    Wc = R.bf(torch.randn(L, H, generator=g) * 0.05)
    bc = torch.randn(L, generator=g).double()
    ref, bound = R.classify_ref(h, Wc, bc)
    assert R.ratio(ref.float(), ref, bound) <= 1                    # f32 output
    wrong, _ = R.classify_ref(h[:, :960], Wc[:, :960], bc)          # the H % 64 tail lost
    assert R.ratio(wrong.float(), ref, bound) > 1
    assert R.ratio(R.rne_bf16(ref), ref, bound) > 1                 # an output rounded to bf16 on the way
