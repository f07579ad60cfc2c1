"""crypto_replace_ffx_fpe_config in the rule compiler (no GPU): which forms are rejected and that each names
its field, that parse_deidentify / Rules without fpe=True keep refusing the primitive, the limits and b(v) of
the alphabet records against big-integer arithmetic, the AES round keys against the reference's, how keys and
alphabets are shared, and that configs without an FPE type compile to the blobs they did before."""
import base64
import hashlib
import json
import os
import re

import numpy as np
import pytest
import yaml

import xform_configs as X
import xform_fpe_ref as FR
import xform_hash_ref as HR
from conftest import ROOT, pkg

NAME = "crypto_replace_ffx_fpe_config"
NAMES = ["EMAIL_ADDRESS", "PHONE_NUMBER"]


def _b64(key):
    return base64.b64encode(key).decode()


def _fpe(**kw):
    cfg = {"crypto_key": {"unwrapped": {"key": _b64(FR.KA)}}, "common_alphabet": "NUMERIC"}
    cfg.update(kw)
    return [{"primitive_transformation": {NAME: {k: v for k, v in cfg.items() if v is not None}}}]


REJECTED = [
    (_fpe(context={"name": "id"}), "context"),
    (_fpe(radix=10, common_alphabet=None), "radix"),
    (_fpe(surrogate_info_type={"name": "TOKEN"}), "surrogate_info_type"),
    (_fpe(crypto_key={"transient": {"name": "k"}}), "crypto_key form transient"),
    (_fpe(crypto_key={"kms_wrapped": {"wrapped_key": "AAAA", "crypto_key_name": "n"}}), "crypto_key form kms_wrapped"),
    (_fpe(crypto_key={"wrapped": {}}), "unknown crypto_key form wrapped"),
    (_fpe(crypto_key=None), "crypto_key is missing"),
    (_fpe(crypto_key={}), "crypto_key is missing"),
    (_fpe(crypto_key={"unwrapped": {}}), "crypto_key.unwrapped.key is missing"),
    (_fpe(crypto_key={"unwrapped": {"key": "not base64!"}}), "crypto_key.unwrapped.key is not base64"),
    (_fpe(crypto_key={"unwrapped": {"key": 5}}), "crypto_key.unwrapped.key is not base64"),
    (_fpe(crypto_key={"unwrapped": {"key": _b64(bytes(20))}}), "crypto_key.unwrapped.key is 20 bytes"),
    (_fpe(crypto_key={"unwrapped": {"key": _b64(bytes(64))}}), "crypto_key.unwrapped.key is 64 bytes"),
    (_fpe(crypto_key={"unwrapped": {"key": _b64(FR.KA), "name": "x"}}), "unwrapped.name"),
    (_fpe(custom_alphabet="01"), "exactly one of common_alphabet and custom_alphabet"),
    (_fpe(common_alphabet=None), "exactly one of common_alphabet and custom_alphabet"),
    (_fpe(common_alphabet="DECIMAL"), "unknown common_alphabet 'DECIMAL'"),
    (_fpe(common_alphabet=None, custom_alphabet="0120"), "custom_alphabet repeats a character"),
    (_fpe(common_alphabet=None, custom_alphabet="01é"), "custom_alphabet character 'é' is not printable ASCII"),
    (_fpe(common_alphabet=None, custom_alphabet="01\t"), "custom_alphabet character '\\t' is not printable ASCII"),
    (_fpe(common_alphabet=None, custom_alphabet="0"), "custom_alphabet does not hold 2 to 95 characters"),
    (_fpe(common_alphabet=None, custom_alphabet=FR.ALPHA95 + "\x7f"), "custom_alphabet does not hold 2 to 95 characters"),
    (_fpe(common_alphabet=None, custom_alphabet=5), "custom_alphabet does not hold 2 to 95 characters"),
    (_fpe(tweak="x"), "unsupported field tweak"),
]


@pytest.mark.parametrize("k", range(len(REJECTED)))
def test_rejected_forms_name_the_field(k):
    comp = pkg("compiler")
    transformations, word = REJECTED[k]
    with pytest.raises(comp.RuleError, match=re.escape(word)) as ei:
        comp.parse_deidentify(X.with_block(transformations), NAMES, fpe=True)
    assert NAME in str(ei.value)


@pytest.fixture(scope="module")
def builtin():
    with open(os.path.join(pkg("compiler").RULES_DIR, "builtin_infotypes.yaml")) as f:
        return yaml.safe_load(f)


def test_without_the_flag_the_primitive_stays_unsupported(builtin, tmp_path):
    comp = pkg("compiler")
    cfg = X.with_block(FR.FC)
    word = "unsupported primitive transformation " + NAME
    with pytest.raises(comp.RuleError, match=word):
        comp.parse_deidentify(cfg, NAMES)
    with pytest.raises(comp.RuleError, match=word):
        comp.parse_deidentify(cfg, NAMES, fpe=False)
    with pytest.raises(comp.RuleError, match=word):
        comp.Rules(cfg, builtin)
    path = X.write(tmp_path, "fc", cfg)
    with pytest.raises(comp.RuleError, match=word):
        comp.Rules.load(path)
    assert {t.kind for t in comp.Rules(cfg, builtin, fpe=True).transforms} == {comp.XF_FPE}
    assert {t.kind for t in comp.Rules.load(path, fpe=True).transforms} == {comp.XF_FPE}
    assert {t.kind for t in comp.compile_default(path).rules.transforms} == {comp.XF_FPE}
    assert NAME in comp._XF_UNSUPPORTED                       # (what the flag-less error is composed from)


def test_accepted_forms():
    comp = pkg("compiler")
    ts = comp.parse_deidentify(X.with_block(_fpe()), NAMES, fpe=True)
    assert [(t.kind, t.key, t.alphabet) for t in ts] == [(comp.XF_FPE, FR.KA, "0123456789")] * 2
    for name, alphabet in FR.COMMON.items():
        t, = comp.parse_deidentify(X.with_block(_fpe(common_alphabet=name)), NAMES[:1], fpe=True)
        assert t.alphabet == alphabet
    t, = comp.parse_deidentify(X.with_block(_fpe(common_alphabet=None, custom_alphabet="zyx !")), NAMES[:1], fpe=True)
    assert t.alphabet == "zyx !"                               # the order given
    t, = comp.parse_deidentify(X.with_block(_fpe(common_alphabet=None, custom_alphabet=FR.ALPHA95)), NAMES[:1], fpe=True)
    assert len(t.alphabet) == 95
    for key in (FR.KA, FR.KB, FR.KC):
        t, = comp.parse_deidentify(X.with_block(_fpe(crypto_key={"unwrapped": {"key": _b64(key)}})), NAMES[:1], fpe=True)
        assert t.key == key


@pytest.mark.parametrize("radix", [2, 3, 9, 10, 16, 36, 62, 95])
def test_alphabet_record_against_big_integers(radix):
    comp = pkg("compiler")
    alphabet = FR.ALPHA95[60:60 + radix] if radix <= 35 else FR.ALPHA95[:radix]
    alphabet = alphabet[::-1]                                   # not in code order
    rec = comp.fpe_alphabet_words(alphabet)
    assert rec.dtype == np.uint32 and len(rec) == comp.XF_FPE_ALPHA_WORDS == 68
    raw = rec.astype("<u4").tobytes()
    nmin = next(n for n in range(2, 200) if radix ** n >= 100)
    vmax = max(v for v in range(1, 200) if radix ** v <= 2 ** 128)
    nmax = min(2 * vmax, 64)
    assert [int(x) for x in rec[:4]] == [radix, nmin, nmax, 0]
    assert (nmin, nmax) == comp.fpe_limits(radix) == FR.limits(radix)
    table = {2: (7, 64), 10: (2, 64), 16: (2, 64), 36: (2, 48), 62: (2, 42), 95: (2, 38)}
    assert radix not in table or table[radix] == (nmin, nmax)
    to_digit, to_byte, bv = raw[16:144], raw[144:240], raw[240:272]
    for c in range(128):
        assert to_digit[c] == (alphabet.index(chr(c)) if chr(c) in alphabet else 0xFF)
    assert to_byte[:radix] == alphabet.encode() and to_byte[radix:] == bytes(96 - radix)
    for v in range(1, 33):
        exact = -(-(radix ** v - 1).bit_length() // 8)
        if 2 * v - 1 <= nmax:                                  # a v that some accepted n has
            assert bv[v - 1] == exact <= 16, v
            assert 4 * -(-exact // 4) + 4 <= 20
        else:
            assert bv[v - 1] == min(exact, 16)
    assert list(bv) == sorted(bv)


@pytest.mark.parametrize("key", [FR.KA, FR.KC, FR.KB, FR.K128, FR.K192, FR.K256], ids=lambda k: str(len(k)))
def test_round_keys_match_the_reference(key):
    comp = pkg("compiler")
    w = comp.aes_round_keys(key)
    assert list(w) == FR.aes_round_keys(key) and len(w) == 4 * (len(key) // 4 + 7)
    rec = comp.fpe_key_words(key)
    assert len(rec) == comp.XF_FPE_KEY_WORDS == 64 and int(rec[0]) == len(key) // 4 + 6
    assert [int(x) for x in rec[1:1 + len(w)]] == list(w) and not rec[1 + len(w):].any()
    # FIPS-197 A.1: the last word of the expanded 2b7e1516... key
    if key == FR.K128:
        assert w[43] == 0xB6630CA6


def test_sections_share_equal_keys_and_alphabets():
    comp = pkg("compiler")
    T = comp.Transform
    ts = [T(comp.XF_FPE, key=FR.KA, alphabet="0123456789"), T(comp.XF_REDACT),
          T(comp.XF_FPE, key=FR.KB, alphabet="0123456789"), T(comp.XF_FPE, key=FR.KA, alphabet="ab"),
          T(comp.XF_INFO_TYPE), T(comp.XF_FPE, key=FR.KB, alphabet="ab")]
    S = comp.transform_sections(ts)
    assert [n for n in S if n.startswith("xf.")] == ["xf.kind", "xf.repl_off", "xf.repl", "xf.mask", "xf.fpe",
                                                     "xf.fpe_key", "xf.fpe_alpha"]
    assert [int(k) for k in S["xf.kind"]] == [6, 2, 6, 6, 0, 6] and comp.XF_FPE == 6
    assert [int(x) for x in S["xf.fpe"]] == [0, 0, 1, 1 << 16, 0, 1 | 1 << 16]
    assert len(S["xf.fpe_key"]) == 2 * 64 and len(S["xf.fpe_alpha"]) == 2 * 68
    assert np.array_equal(S["xf.fpe_key"][64:], comp.fpe_key_words(FR.KB))
    assert np.array_equal(S["xf.fpe_alpha"][68:], comp.fpe_alphabet_words("ab"))
    assert not S["xf.repl_off"].any()                          # xf.repl gets nothing for an FPE type
    many = [T(comp.XF_FPE, key=bytes([i]) * 16, alphabet="01") for i in range(17)]
    with pytest.raises(comp.RuleError, match="more than 16 distinct keys"):
        comp.transform_sections(many)
    assert len(comp.transform_sections(many[:16])["xf.fpe_key"]) == 16 * 64


def test_config_f_sections(tmp_path, compiled):
    comp = pkg("compiler")
    c = comp.compile_default(X.write(tmp_path, "F", X.with_block(FR.F)))
    S, names = c.sections, c.rules.type_names
    want = {n: comp.XF_FPE for n in FR.F_FPE}
    want["SOCIAL_HANDLE"] = comp.XF_REDACT
    assert [int(k) for k in S["xf.kind"]] == [want.get(n, comp.XF_INFO_TYPE) for n in names]
    ka = {n: (int(S["xf.fpe"][t]) & 0xFFFF, int(S["xf.fpe"][t]) >> 16) for t, n in enumerate(names) if n in FR.F_FPE}
    groups = ((FR.F_NUMERIC, FR.KA, "NUMERIC"), (FR.F_UPPER, FR.KC, "UPPER_CASE_ALPHA_NUMERIC"),
              (("EMAIL_ADDRESS",), FR.KB, "ALPHA_NUMERIC"))
    assert len(set(ka.values())) == 3
    for types, key, alpha in groups:
        (k, a), = {ka[n] for n in types}
        assert np.array_equal(S["xf.fpe_key"][64 * k:64 * k + 64], comp.fpe_key_words(key))
        assert np.array_equal(S["xf.fpe_alpha"][68 * a:68 * a + 68], comp.fpe_alphabet_words(FR.COMMON[alpha]))
    assert [int(x) for t, x in enumerate(S["xf.fpe"]) if names[t] not in FR.F_FPE] == [0] * (len(names) - len(FR.F_FPE))
    assert len(S["xf.fpe_key"]) == 3 * 64 and len(S["xf.fpe_alpha"]) == 3 * 68
    for n, a in compiled.sections.items():                      # everything else is the shipped blob's
        assert np.array_equal(S[n], a), n
    assert "xf.hash_key" not in S
    for secret in (base64.b64encode(FR.KA), base64.b64encode(FR.KB), base64.b64encode(FR.KC)):
        assert c.blob.count(secret) == 0


def test_blobs_without_an_fpe_type_are_the_parents(tmp_path):
    comp = pkg("compiler")
    with open(os.path.join(ROOT, "tests", "golden", "fpe_parent_blob_sha256.json")) as f:
        golden = json.load(f)
    absent = X.shipped()
    del absent["deidentify_config"]
    cfgs = {"shipped": X.shipped(), "no_block": absent, "A": X.with_block(X.A), "B": X.with_block(X.B),
            "C": X.with_block(X.C), "H": X.with_block(HR.H), "HC": X.with_block(HR.HC)}
    assert set(cfgs) == set(golden) - {"_what"}
    for n, cfg in cfgs.items():
        c = comp.compile_default(X.write(tmp_path, n, cfg))
        assert hashlib.sha256(c.blob).hexdigest() == golden[n], n
        assert not [s for s in c.sections if s.startswith("xf.fpe")]


def test_header_layout_and_engine_mirror_the_constants():
    E, comp = pkg("engine"), pkg("compiler")
    src = open(os.path.join(ROOT, "include", "pii_engine.h")).read()
    assert re.search(r"^#define PII_XF_FPE 6$", src, re.M)
    assert E.PII_XF_FPE == comp.XF_FPE == 6
    lay = open(os.path.join(ROOT, "context-based-pii_amd", "csrc", "pii_layout.h")).read()
    for name in ("KEY_WORDS", "ALPHA_WORDS", "NMAX", "KEYS_MAX"):
        m = re.search(rf"^constexpr int XF_FPE_{name} = (\d+);", lay, re.M)
        assert m and int(m.group(1)) == getattr(comp, "XF_FPE_" + name), name
