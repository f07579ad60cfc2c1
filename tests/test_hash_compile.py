"""crypto_hash_config in the rule compiler (no GPU): the compiler's own SHA-256 compression and the HMAC
midstates it emits against hmac / hashlib, literal known answers, how parse_deidentify resolves hash
types and keys, which forms are rejected, and that configs without a hash type compile to the blob they
always did."""
import base64
import hashlib
import hmac
import os
import re
import struct

import numpy as np
import pytest

import xform_configs as X
import xform_hash_ref as HR
from conftest import ROOT, pkg

LENGTHS = (1, 55, 56, 63, 64, 65, 119, 120, 1000)


def _compile(cfg: dict):
    comp = pkg("compiler")
    with open(os.path.join(comp.RULES_DIR, "builtin_infotypes.yaml")) as f:
        import yaml
        builtin = yaml.safe_load(f)
    return comp.compile_rules(comp.Rules(cfg, builtin))


def _finish(state, msg: bytes, before: int) -> bytes:
    """SHA-256 of `before` already-compressed bytes (chaining value `state`) followed by msg"""
    comp = pkg("compiler")
    data = msg + b"\x80" + b"\0" * ((55 - len(msg)) % 64) + struct.pack(">Q", (before + len(msg)) * 8)
    assert len(data) % 64 == 0 and len(data) // 64 == (len(msg) + 9 + 63) // 64
    for b in range(0, len(data), 64):
        state = comp.sha256_compress(state, data[b:b + 64])
    return struct.pack(">8I", *state)


def _hmac_from_midstates(mid, msg: bytes) -> bytes:
    """what the engine computes: mid = 16 words, the inner then the outer midstate"""
    inner = _finish(tuple(int(w) for w in mid[:8]), msg, 64)
    return _finish(tuple(int(w) for w in mid[8:]), inner, 64)


@pytest.fixture(scope="module")
def compiled_h():
    return _compile(X.with_block(HR.H))


def test_compression_function_is_sha256():
    comp = pkg("compiler")
    for n in (0,) + LENGTHS:
        msg = bytes((7 * i + 3) & 255 for i in range(n))
        assert _finish(comp.SHA256_IV, msg, 0) == hashlib.sha256(msg).digest(), n


@pytest.mark.parametrize("key", [HR.KEY1, HR.KEY2], ids=["key32", "key64"])
@pytest.mark.parametrize("n", LENGTHS)
def test_emitted_midstates_finish_to_hmac(key, n):
    comp = pkg("compiler")
    S = comp.transform_sections([comp.Transform(comp.XF_HASH, key=key)])
    mid = S["xf.hash_mid"]
    assert mid.dtype == np.uint32 and len(mid) == comp.XF_HASH_KEY_WORDS == 16
    msg = bytes((11 * i + n) & 255 for i in range(n))
    assert _hmac_from_midstates(mid, msg) == hmac.new(key, msg, hashlib.sha256).digest()


def test_literal_known_answers():
    comp = pkg("compiler")
    assert base64.b64encode(HR.KEY1) == b"AAECAwQFBgcICQoLDA0ODxAREhMUFRYXGBkaGxwdHh8="
    for key, msg, want in ((HR.KEY1, HR.CARD, HR.CARD_KEY1), (HR.KEY1, HR.SSN, HR.SSN_KEY1),
                           (HR.KEY2, HR.SSN, HR.SSN_KEY2), (HR.KEY1, "José Núñez".encode(), HR.JOSE_KEY1)):
        assert len(want) == 44
        assert HR.surrogate(key, msg) == want
        mid = [w for m in comp.hmac_midstates(key) for w in m]
        assert base64.b64encode(_hmac_from_midstates(mid, msg)) == want
    assert HR.CARD == b"4111 1111 1111 1111" and HR.SSN == b"536-22-1234"


def test_reference_helper_extends_xform_ref(oracle_cfg):
    from oracle import pii_oracle as O
    import xform_ref
    names = oracle_cfg.type_names
    text = b"my ssn is 536-22-1234@johnny thanks"
    fs = O.find_pii(text, oracle_cfg)
    assert [(f.start, f.end) for f in fs] == [(10, 21), (21, 28)]
    assert HR.apply_transform(text, fs, names, X.with_block(HR.H)) == b"my ssn is " + HR.SSN_KEY1 + b" thanks"
    assert HR.apply_transform(text, fs, names, X.with_block(HR.HC)) == (
        b"my ssn is " + HR.SSN_KEY1 + HR.surrogate(HR.KEY1, b"@johnny") + b" thanks")
    # without a hash type it is xform_ref
    for block in (X.A, X.B, X.C, None):
        for t, _ in X.KNOWN_A:
            f = O.find_pii(t, oracle_cfg)
            cfg = X.with_block(block)
            assert HR.apply_transform(t, f, names, cfg) == xform_ref.apply_transform(t, f, names, cfg)


def test_parse_resolves_listed_catch_all_and_first_entry_wins():
    comp = pkg("compiler")
    names = ["EMAIL_ADDRESS", "PHONE_NUMBER", "IP_ADDRESS"]

    def parse(transformations):
        return comp.parse_deidentify(X.with_block(transformations), names)

    ts = parse([{"info_types": [{"name": "PHONE_NUMBER"}], "primitive_transformation": HR.hash_prim(HR.KEY2)}])
    assert [t.kind for t in ts] == [comp.XF_KEEP, comp.XF_HASH, comp.XF_KEEP] and ts[1].key == HR.KEY2
    ts = parse(HR.HC)
    assert [t.kind for t in ts] == [comp.XF_HASH] * 3 and {t.key for t in ts} == {HR.KEY1}
    ts = parse([{"info_types": [{"name": "EMAIL_ADDRESS"}], "primitive_transformation": HR.hash_prim(HR.KEY1)},
                {"info_types": [{"name": "EMAIL_ADDRESS"}, {"name": "IP_ADDRESS"}],
                 "primitive_transformation": X._mask(masking_character="*")}])
    assert [t.kind for t in ts] == [comp.XF_HASH, comp.XF_KEEP, comp.XF_MASK]
    ts = parse([{"info_types": [{"name": "EMAIL_ADDRESS"}], "primitive_transformation": X._mask()},
                {"info_types": [{"name": "EMAIL_ADDRESS"}], "primitive_transformation": HR.hash_prim(HR.KEY1)}])
    assert [t.kind for t in ts] == [comp.XF_MASK, comp.XF_KEEP, comp.XF_KEEP]


def test_key_indices_one_per_distinct_key():
    comp = pkg("compiler")
    T = comp.Transform
    S = comp.transform_sections([T(comp.XF_HASH, key=HR.KEY1), T(comp.XF_REDACT), T(comp.XF_HASH, key=HR.KEY1)])
    assert [int(k) for k in S["xf.hash_key"]] == [0, 0, 0] and len(S["xf.hash_mid"]) == 16
    S = comp.transform_sections([T(comp.XF_HASH, key=HR.KEY2), T(comp.XF_HASH, key=HR.KEY1),
                                 T(comp.XF_INFO_TYPE), T(comp.XF_HASH, key=HR.KEY2)])
    assert S["xf.hash_key"].dtype == np.uint32
    assert [int(k) for k in S["xf.hash_key"]] == [0, 1, 0, 0] and len(S["xf.hash_mid"]) == 32
    for k, key in enumerate((HR.KEY2, HR.KEY1)):
        want = [w for m in comp.hmac_midstates(key) for w in m]
        assert [int(w) for w in S["xf.hash_mid"][16 * k:16 * k + 16]] == want


def _h(cfg):
    return [{"primitive_transformation": {"crypto_hash_config": cfg}}]


_B64 = base64.b64encode(HR.KEY1).decode()
REJECTED = [
    (_h({"crypto_key": {"transient": {"name": "k"}}}), "transient"),
    (_h({"crypto_key": {"kms_wrapped": {"wrapped_key": _B64, "crypto_key_name": "projects/p"}}}), "kms_wrapped"),
    (_h({}), "crypto_key"),
    (_h(None), "crypto_key"),
    (_h({"crypto_key": {}}), "crypto_key"),
    (_h({"crypto_key": {"unwrapped": {}}}), "unwrapped.key"),
    (_h({"crypto_key": {"unwrapped": {"key": "not base64!"}}}), "unwrapped.key is not base64"),
    (_h({"crypto_key": {"unwrapped": {"key": 7}}}), "unwrapped.key is not base64"),
    (_h({"crypto_key": {"unwrapped": {"key": base64.b64encode(bytes(16)).decode()}}}), "unwrapped.key is 16 bytes"),
    (_h({"crypto_key": {"unwrapped": {"key": base64.b64encode(bytes(48)).decode()}}}), "unwrapped.key is 48 bytes"),
    (_h({"crypto_key": {"unwrapped": {"key": ""}}}), "unwrapped.key is 0 bytes"),
    (_h({"crypto_key": {"unwrapped": {"key": _B64}}, "surrogate_info_type": {"name": "X"}}), "surrogate_info_type"),
    (_h({"crypto_key": {"unwrapped": {"key": _B64, "salt": "x"}}}), "salt"),
    (_h({"crypto_key": {"unwrapped": {"key": _B64}, "transient": {"name": "k"}}}), "transient"),
    # the other crypto / bucketing primitives stay rejected
    ([{"primitive_transformation": {"crypto_deterministic_config": {}}}], "unsupported primitive transformation crypto_d"),
    ([{"primitive_transformation": {"crypto_replace_ffx_fpe_config": {}}}], "unsupported primitive transformation"),
    ([{"primitive_transformation": {"date_shift_config": {}}}], "unsupported primitive transformation"),
    ([{"primitive_transformation": {"bucketing_config": {}}}], "unsupported primitive transformation"),
    ([{"primitive_transformation": {"fixed_size_bucketing_config": {}}}], "unsupported primitive transformation"),
    ([{"primitive_transformation": {"time_part_config": {}}}], "unsupported primitive transformation"),
    ([{"primitive_transformation": {"replace_dictionary_config": {}}}], "unsupported primitive transformation"),
]


@pytest.mark.parametrize("k", range(len(REJECTED)))
def test_rejected_forms_name_the_field(k):
    comp = pkg("compiler")
    transformations, word = REJECTED[k]
    with pytest.raises(comp.RuleError, match=re.escape(word)):
        comp.parse_deidentify(X.with_block(transformations), ["EMAIL_ADDRESS", "PHONE_NUMBER"])


def test_blob_unchanged_without_a_hash_type(compiled):
    """the shipped config, no block at all and blocks A / B / C / D: no hash section, and the blob is the
    shipped sections followed by exactly the four xf.* sections the transformation work defined"""
    comp = pkg("compiler")
    absent = X.shipped()
    del absent["deidentify_config"]
    for cfg in (X.shipped(), absent):
        assert _compile(cfg).blob == compiled.blob
    assert not [n for n in compiled.sections if n.startswith("xf.")]
    D = [{"info_types": [{"name": "EMAIL_ADDRESS"}],
          "primitive_transformation": {"replace_config": {"new_value": {"string_value": "<email>"}}}},
         {"info_types": [{"name": "SOCIAL_HANDLE"}], "primitive_transformation": {"redact_config": {}}},
         {"primitive_transformation": {"replace_with_info_type_config": {}}}]
    for block in (X.A, X.B, X.C, D):
        c = _compile(X.with_block(block))
        assert [n for n in c.sections if n.startswith("xf.")] == ["xf.kind", "xf.repl_off", "xf.repl", "xf.mask"]
        assert max(int(k) for k in c.sections["xf.kind"]) <= comp.XF_KEEP
        # rebuilt from the shipped sections and the transforms alone, as before this kind existed
        S = type(compiled.sections)(compiled.sections)
        T = len(c.rules.type_names)
        ts = c.rules.transforms
        S["xf.kind"] = np.array([t.kind for t in ts], dtype=np.uint8)
        S["xf.repl_off"] = np.cumsum([0] + [len(t.value) for t in ts]).astype(np.uint32)
        S["xf.repl"] = np.frombuffer(b"".join(t.value for t in ts) or b"\0", dtype=np.uint8).copy()
        S["xf.mask"] = c.sections["xf.mask"]
        assert len(S["xf.mask"]) == T * comp.XF_MASK_WORDS
        assert comp._sections_to_blob(S) == c.blob


def test_hash_config_carries_the_new_sections(compiled, compiled_h):
    comp = pkg("compiler")
    S = comp.blob_sections(compiled_h.blob)
    names = compiled_h.rules.type_names
    T = len(names)
    assert [n for n in S if n.startswith("xf.")] == ["xf.kind", "xf.repl_off", "xf.repl", "xf.mask", "xf.hash_key",
                                                     "xf.hash_mid"]
    for n, a in compiled.sections.items():
        assert np.array_equal(S[n], a), n
    want = {n: comp.XF_HASH for n in HR.H_HASHED}
    want["SOCIAL_HANDLE"] = comp.XF_REDACT
    assert comp.XF_HASH == 5
    assert [int(k) for k in S["xf.kind"]] == [want.get(n, comp.XF_INFO_TYPE) for n in names]
    off, repl = S["xf.repl_off"], S["xf.repl"].tobytes()
    for t, n in enumerate(names):
        assert repl[int(off[t]):int(off[t + 1])] == (b"=" * 44 if n in HR.H_HASHED else b""), n
    key = S["xf.hash_key"]
    assert len(key) == T and len(S["xf.hash_mid"]) == 32
    assert {n: int(key[t]) for t, n in enumerate(names) if n in HR.H_HASHED} == {
        "CREDIT_CARD_NUMBER": 0, "US_SOCIAL_SECURITY_NUMBER": 0, "EMAIL_ADDRESS": 0, "PHONE_NUMBER": 1}
    assert base64.b64encode(_hmac_from_midstates(S["xf.hash_mid"][:16], HR.CARD)) == HR.CARD_KEY1
    assert base64.b64encode(_hmac_from_midstates(S["xf.hash_mid"][16:], HR.SSN)) == HR.SSN_KEY2
    # the raw keys are not in the blob (nor their base64 form)
    for secret in (HR.KEY1, HR.KEY2[32:], base64.b64encode(HR.KEY1), base64.b64encode(HR.KEY2)):
        assert compiled_h.blob.count(secret) == compiled.blob.count(secret) == 0


def test_header_and_engine_export_the_kind():
    E, comp = pkg("engine"), pkg("compiler")
    src = open(os.path.join(ROOT, "include", "pii_engine.h")).read()
    assert re.search(r"^#define PII_XF_HASH 5$", src, re.M)
    assert E.PII_XF_HASH == comp.XF_HASH == 5
