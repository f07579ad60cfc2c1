"""Optional NER detector: bf16 BERT-base token classification on MFMA
(csrc/ner.hip) vs the same HF model in fp32 on the CPU (transformers.BertConfig(), seeded random
weights, nothing fetched).  Per op: a float64 reference on the bf16-rounded inputs under the derived
per-element bounds of tests/ner_ref.py (tests/test_gpu_ner_ops.py covers the ops' other paths and
edges); for the whole 12-layer model: the logits (relative L2 error and argmax agreement)."""
import numpy as np
import pytest

from conftest import pkg


def test_tokenizer_and_span_decoding():
    N = pkg("ner")
    tok = N.HashTokenizer(max_len=16)
    ids, spans = tok.encode(b"My name is John Smith, ok?")
    assert ids[0] == N.CLS and ids[-1] == N.SEP and len(ids) == len(spans)
    assert [b"My name is John Smith, ok?"[s:e] for s, e in spans[1:-1]] == [b"My", b"name", b"is", b"John", b"Smith",
                                                                           b",", b"ok", b"?"]
    assert tok.encode(b"JOHN")[0][1] == tok.encode(b"john")[0][1]               # case-folded
    assert all(1000 <= i < 30522 for i in ids[1:-1])
    B, M, S = tok.batch([b"a b", b"x" * 3 + b" y" * 40])
    assert B.shape == (2, 16) and M[0].sum() == 4 and M[1].sum() == 16         # truncated to max_len
    # BIO: [CLS] My name is John Smith , ok ? [SEP]
    lab = [0, 0, 0, 0, 1, 2, 0, 0, 0, 0]
    assert N.decode_spans(lab, spans) == [(11, 21)]
    assert N.decode_spans([0, 2, 2, 0, 1, 1, 0, 0, 0, 0], spans) == [(0, 7), (11, 15), (16, 21)]


@pytest.fixture(scope="module")
def ner_model():
    N = pkg("ner")
    ref = N.reference_model(seed=3)
    return ref, N.BertNer(ref, device=0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 192), (1024, 2304, 768), (512, 768, 3072)])
def test_gemm_vs_torch(ner_model, M, N, K):
    """each element inside the derived bound of tests/ner_ref.py: one bf16 ulp of output rounding plus the
    f32 accumulation term (plus gelu_erf's own error under GELU)"""
    import torch
    import ner_ref as R
    Nm = pkg("ner")
    _, m = ner_model
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    Rs = torch.randn(M, N, generator=g).to(torch.bfloat16)
    dev = m.dev
    Ab, Wb, Rb = (x.to(dev) for x in (A, W, Rs))
    for epi in (Nm.EPI_BIAS, Nm.EPI_GELU, Nm.EPI_RESID):
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        m.gemm(Ab, Wb, bias.to(dev), out, epi, resid=Rb if epi == Nm.EPI_RESID else None)
        r = R.gemm_ratio(out.cpu(), A, W, bias, Rs, epi)
        print("ner_ratio gemm", (M, N, K), epi, r)
        assert r <= 1, (epi, r)


@pytest.mark.gpu
def test_layernorm_and_attention_vs_torch(ner_model):
    import torch
    import ner_ref as R
    _, m = ner_model
    dev = m.dev
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(256, 768, generator=g) * 3 + 1).to(torch.bfloat16)
    gam, bet = torch.randn(768, generator=g), torch.randn(768, generator=g)
    out = torch.empty(256, 768, dtype=torch.bfloat16, device=dev)
    m.layernorm(x.to(dev), gam.to(dev), bet.to(dev), out)
    want, xhat = R.layernorm_ref(x, gam, bet, m.eps)
    r = R.ratio(out.cpu(), want, R.layernorm_bound(want, xhat, gam, bet))
    print("ner_ratio layernorm", r)
    assert r <= 1, r
    # attention over the fused QKV rows, with padded keys masked: the matrix-core kernel (S % 32 == 0,
    # S <= 128) and the general one
    for B, S in ((2, 64), (3, 128), (2, 48), (1, 160)):
        Hh = 12
        qkv = torch.randn(B * S, 3 * 768, generator=g).to(torch.bfloat16)
        mask = torch.ones(B, S, dtype=torch.int32)
        mask[-1, S * 5 // 8:] = 0
        ctx = torch.zeros(B * S, 768, dtype=torch.bfloat16, device=dev)
        rc = m.lib.ner_attention(qkv.to(dev).data_ptr(), mask.to(dev).data_ptr(), ctx.data_ptr(), B, S, Hh, 64, m._st())
        assert rc == 0
        want, absv = R.attention_ref(qkv, mask, B, S, Hh)
        r = R.ratio(ctx.cpu(), want, R.attention_bound(want, absv, R.attention_is_mfma(S)))
        print("ner_ratio attention", (B, S), r)
        assert r <= 1, (S, r)


@pytest.mark.gpu
def test_bert_logits_vs_hf_cpu(ner_model):
    """the whole 12-layer model vs HF fp32 on the CPU, same ids and mask (ragged lengths)"""
    import torch
    Nm = pkg("ner")
    ref, m = ner_model
    tok = Nm.HashTokenizer(max_len=64)
    texts = [b"my name is john smith and i live on main street", b"ok", b"please call jane doe at home " * 3,
             b"the account holder is Maria Garcia-Lopez, date of birth 01/02/1980"]
    ids, mask, _ = tok.batch(texts)
    got = m.forward(ids, mask).float().cpu()
    with torch.no_grad():
        want = ref(input_ids=torch.as_tensor(ids, dtype=torch.long),
                   attention_mask=torch.as_tensor(mask, dtype=torch.long)).logits
    sel = torch.as_tensor(mask, dtype=torch.bool)
    g, w = got[sel], want[sel]
    rel = ((g - w).norm() / w.norm()).item()
    agree = (g.argmax(-1) == w.argmax(-1)).float().mean().item()
    assert rel < 0.05 and agree > 0.9, (rel, agree)
