"""float64 references and derived error bounds for the NER ops of csrc/ner.hip (no GPU needed).

Every reference is computed in float64 on the bf16-rounded inputs (callers pass tensors that already
hold bf16 values; anything else is widened as it is).  The bounds are derived from the number formats
and the kernels' arithmetic, not tuned to what the kernels give:

  GEMM            ulp_bf16(ref) + 2^-22 (sum_k |a w| + |bias| + |r|)       output rounding + f32 accumulation
  GEMM + GELU     ... + 3e-7 |v|   0.5 |v| x (1.5e-7 A&S 7.1.26 + ~2 ulp rcpf + ~2 ulp __expf, terms <= 1)
  LayerNorm/embed ulp_bf16(ref) + 1e-5 (|gamma xhat| + |beta|)
  classify        2^-21 (sum_k |h w| + |bc|)                               f32 output, no output rounding
  attention       ulp_bf16(ref) + 2^-20 absv   (k_attention: f32 probabilities)
                  ulp_bf16(ref) + 2^-8 absv    (k_attention_mfma: P rounded to bf16 for the second MFMA)
                  with absv = the softmax-weighted mean of |V|

Each comparator returns the worst |got - ref| / bound, so a test asserts ratio <= 1 and the margin can
be recorded.  tests/test_ner_ref.py shows on the CPU that each bound passes the rounded reference and
fails a subtly wrong computation.
"""
import math

import torch

F64 = torch.float64
EPI_BIAS, EPI_GELU, EPI_RESID = 0, 1, 2
BF16_MIN_EXP = -126            # exponent of the smallest normal; subnormals share its ulp, 2^-133


def f64(t):
    """any tensor / array / scalar as a float64 CPU tensor (bf16 and f32 widen exactly)"""
    return torch.as_tensor(t).detach().cpu().to(F64)


def bf(t):
    """t rounded to bf16 (torch's cast) and widened to float64: how the tests make their inputs"""
    return torch.as_tensor(t).to(torch.bfloat16).to(F64)


def _pow2(k):
    """2^k as float64 for an int64 tensor k in [-1022, 1023], exact (built from the exponent field)"""
    return ((k + 1023) << 52).view(F64)


def _floor_log2(x):
    """floor(log2 |x|) clamped below at BF16_MIN_EXP (0 and subnormals land there); int64"""
    _, e = torch.frexp(x)                  # |x| = m 2^e, 0.5 <= m < 1
    e = torch.where(x == 0, torch.full_like(e, BF16_MIN_EXP), e - 1)      # (frexp(0) = (0, 0))
    return torch.clamp(e.to(torch.int64), min=BF16_MIN_EXP, max=1000)


def ulp_bf16(x):
    """the bf16 ulp at x (8 significand bits): 2^(floor(log2 |x|) - 7), 2^-133 at and below the
    smallest normal, inf where x is not finite"""
    x = f64(x)
    u = _pow2(_floor_log2(torch.where(torch.isfinite(x), x, torch.zeros_like(x))) - 7)
    return torch.where(torch.isfinite(x), u, torch.full_like(x, math.inf))


def rne_bf16(x):
    """the correctly rounded (nearest, ties to even) bf16 of float64 x, as float64; overflow -> inf"""
    x = f64(x)
    fin = torch.isfinite(x)
    xs = torch.where(fin, x, torch.zeros_like(x))
    k = _floor_log2(xs) - 7
    r = torch.round(xs * _pow2(-k)) * _pow2(k)        # both scalings exact; torch.round is half-to-even
    r = torch.where(r.abs() >= 2.0 ** 128, torch.copysign(torch.full_like(r, math.inf), r), r)
    return torch.where(fin, r, x)


def trunc_bf16(x):
    """x chopped to bf16 (round toward zero): the wrong rounding the exact tests must catch"""
    x = f64(x)
    k = _floor_log2(x) - 7
    return torch.trunc(x * _pow2(-k)) * _pow2(k)


def bf16_bits(t):
    """bf16 bit patterns as an int32 tensor: of a bf16 tensor as stored, or of a float tensor whose
    values are exactly representable in bf16 (such as rne_bf16's result)"""
    t = torch.as_tensor(t).detach().cpu()
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    f = t.to(torch.float32)
    if not torch.equal(f.to(F64).nan_to_num(1.0, 2.0, 3.0), t.to(F64).nan_to_num(1.0, 2.0, 3.0)):
        raise ValueError("not exactly representable in f32")
    b = f.contiguous().view(torch.int32)
    if bool((b & 0xFFFF).ne(0).logical_and(torch.isfinite(f)).any()):
        raise ValueError("not exactly representable in bf16")
    return (b >> 16) & 0xFFFF


def _bits_of_rounded(x):
    """bf16_bits of rne_bf16's result without the representability checks (true by construction)"""
    return (x.to(torch.float32).view(torch.int32) >> 16) & 0xFFFF


def ratio(got, ref, bound):
    """worst |got - ref| / bound; inf if a non-finite reference value is not reproduced or got has a
    non-finite value the reference has not"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    fin = torch.isfinite(ref)
    if bool(fin.all()):                            # (the usual case, kept cheap for the largest shapes)
        q = (got - ref).abs() / bound
        return float(q.max()) if bool(torch.isfinite(got).all()) else math.inf
    same = torch.where(fin, torch.isfinite(got), (got == ref) | (torch.isnan(got) & torch.isnan(ref)))
    if not bool(same.all()):
        return math.inf
    if not bool(fin.any()):
        return 0.0
    return float(((got - ref).abs()[fin] / bound[fin]).max())


# --------------------------------------------------------------------------------------------- GEMM
def gelu_erf(v):
    return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))


def gelu_tanh(v):
    """the tanh approximation: the wrong GELU the bound must catch"""
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def gemm_ref(A, W, bias, R, epi):
    """(v, result): v = A . W^T + bias, result = v | gelu_erf(v) | v + R.  bias / R may be None."""
    A, W = f64(A), f64(W)
    v = A @ W.T
    if bias is not None:
        v = v + f64(bias)
    if epi == EPI_GELU:
        return v, gelu_erf(v)
    if epi == EPI_RESID:
        return v, v + f64(R)
    return v, v


def gemm_bound(A, W, bias, R, epi, v, ref):
    mag = f64(A).abs() @ f64(W).abs().T
    if bias is not None:
        mag = mag + f64(bias).abs()
    if epi == EPI_RESID:
        mag = mag + f64(R).abs()
    b = ulp_bf16(ref) + 2.0 ** -22 * mag
    if epi == EPI_GELU:
        b = b + 3e-7 * v.abs()
    return b


def _row_chunks(M, rows):
    return [(i, min(i + rows, M)) for i in range(0, M, rows)]


def gemm_ratio(got, A, W, bias, R, epi, rows=1024):
    """worst error-to-bound ratio of got [M, N] under the real-valued GEMM bound, in row chunks (the
    float64 images of the largest shape would not fit at once)"""
    worst = 0.0
    for lo, hi in _row_chunks(A.shape[0], rows):
        r = R[lo:hi] if R is not None else None
        v, ref = gemm_ref(A[lo:hi], W, bias, r, epi)
        worst = max(worst, ratio(got[lo:hi], ref, gemm_bound(A[lo:hi], W, bias, r, epi, v, ref)))
    return worst


def gemm_exact(got, A, W, bias, R, epi, rows=1024):
    """(mismatches, big): how many elements of the bf16 tensor got differ in bits from rne_bf16 of the
    float64 result, and the fraction of reference results above 256 in magnitude (where bf16 no longer
    holds every integer, so the rounding and its ties are exercised)"""
    bad, big, n = 0, 0, 0
    for lo, hi in _row_chunks(A.shape[0], rows):
        _, ref = gemm_ref(A[lo:hi], W, bias, R[lo:hi] if R is not None else None, epi)
        bad += int((bf16_bits(got[lo:hi]) != _bits_of_rounded(rne_bf16(ref))).sum())
        big += int((ref.abs() > 256).sum())
        n += ref.numel()
    return bad, big / n


# ------------------------------------------------------------------------- LayerNorm, embed, classify
def layernorm_ref(x, gamma, beta, eps):
    """(result, xhat) per row of x [M, H]"""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    xhat = (x - mean) / torch.sqrt(var + eps)
    return xhat * gamma + beta, xhat


def layernorm_bound(ref, xhat, gamma, beta):
    return ulp_bf16(ref) + 1e-5 * ((f64(gamma) * xhat).abs() + f64(beta).abs())


def embed_sum(ids, wemb, pemb, temb, S):
    """word[id] + pos[row % S] + type0 per row"""
    ids = torch.as_tensor(ids).cpu().long()
    pos = torch.arange(ids.numel()) % S
    return f64(wemb)[ids] + f64(pemb)[pos] + f64(temb)


def embed_ref(ids, wemb, pemb, temb, gamma, beta, S, eps):
    return layernorm_ref(embed_sum(ids, wemb, pemb, temb, S), gamma, beta, eps)


def classify_ref(h, Wc, bc):
    """(logits [M, L], bound)"""
    h, Wc, bc = f64(h), f64(Wc), f64(bc)
    return h @ Wc.T + bc, 2.0 ** -21 * (h.abs() @ Wc.abs().T + bc.abs())


# ---------------------------------------------------------------------------------------- attention
def attention_ref(qkv, mask, B, S, heads, d=64):
    """(out, absv) [B*S, heads*d] from the fused rows qkv [B*S, 3*heads*d] (Q | K | V, head major):
    out = softmax(Q K^T / sqrt(d) over the kept keys) V, absv = the same weights over |V|.  mask
    [B, S] (nonzero = kept) or None; a sequence with no kept key is all zeros."""
    H = heads * d
    x = f64(qkv).reshape(B, S, 3, heads, d)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))            # [B, heads, S, d]
    keep = torch.ones(B, S, dtype=torch.bool) if mask is None else torch.as_tensor(mask).cpu().reshape(B, S) != 0
    sc = q @ k.transpose(-1, -2) / math.sqrt(d)
    sc = sc.masked_fill(~keep[:, None, None, :], -math.inf)
    mx = sc.max(-1, keepdim=True).values
    p = torch.exp(sc - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))   # all masked: exp(-inf) = 0
    l = p.sum(-1, keepdim=True)
    p = torch.where(l > 0, p / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(p))
    out = (p @ v).transpose(1, 2).reshape(B * S, H)
    absv = (p @ v.abs()).transpose(1, 2).reshape(B * S, H)
    return out, absv


def attention_bound(ref, absv, mfma):
    return ulp_bf16(ref) + (2.0 ** -8 if mfma else 2.0 ** -20) * absv


def attention_is_mfma(S):
    """ner_attention's path: the matrix-core kernel for S % 32 == 0, S <= 128, else the general one"""
    return S <= 128 and S % 32 == 0
