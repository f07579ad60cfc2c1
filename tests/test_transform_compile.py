"""deidentify_config in the rule compiler (no GPU): which configs add the xf.* blob sections, what they
hold, which forms are rejected, and the pure-Python reference (xform_ref) against the literal known
answers the GPU tests use."""
import copy
import os
import re

import numpy as np
import pytest

import xform_configs as X
import xform_ref
from conftest import ROOT, pkg


def _compile(cfg: dict):
    comp = pkg("compiler")
    with open(os.path.join(comp.RULES_DIR, "builtin_infotypes.yaml")) as f:
        import yaml
        builtin = yaml.safe_load(f)
    return comp.compile_rules(comp.Rules(cfg, builtin))


def test_info_type_for_all_emits_no_sections(compiled):
    assert not [n for n in compiled.sections if n.startswith("xf.")]
    explicit = X.with_block([{"primitive_transformation": {"replace_with_info_type_config": {}}}])
    listed = X.with_block([{"info_types": [{"name": "EMAIL_ADDRESS"}],
                            "primitive_transformation": {"replace_with_info_type_config": {}}},
                           {"primitive_transformation": {"replace_with_info_type_config": {}}}])
    absent = X.shipped()
    del absent["deidentify_config"]
    for cfg in (explicit, listed, absent):
        c = _compile(cfg)
        assert not [n for n in c.sections if n.startswith("xf.")]
        assert c.blob == compiled.blob


def test_config_a_round_trips_through_blob_sections(compiled):
    comp = pkg("compiler")
    c = _compile(X.with_block(X.A))
    S = comp.blob_sections(c.blob)
    names = c.rules.type_names
    T = len(names)
    # every section of the shipped blob is unchanged; the transformation sections follow
    assert [n for n in S if not n.startswith("xf.")] == list(compiled.sections)
    for n, a in compiled.sections.items():
        assert np.array_equal(S[n], a), n
    kind = S["xf.kind"]
    assert kind.dtype == np.uint8 and len(kind) == T
    want = {"CREDIT_CARD_NUMBER": comp.XF_MASK, "US_SOCIAL_SECURITY_NUMBER": comp.XF_MASK,
            "PHONE_NUMBER": comp.XF_MASK, "EMAIL_ADDRESS": comp.XF_REPLACE, "SOCIAL_HANDLE": comp.XF_REDACT}
    assert [int(k) for k in kind] == [want.get(n, comp.XF_KEEP) for n in names]
    off, repl = S["xf.repl_off"], S["xf.repl"].tobytes()
    assert len(off) == T + 1
    for t, n in enumerate(names):
        assert repl[int(off[t]):int(off[t + 1])] == (b"<email>" if n == "EMAIL_ADDRESS" else b"")
    m = S["xf.mask"].reshape(T, comp.XF_MASK_WORDS)

    def skipset(row):
        return {chr(b) for b in range(128) if (int(row[2 + b // 32]) >> (b % 32)) & 1}

    card, ssn, phone = (m[names.index(n)] for n in ("CREDIT_CARD_NUMBER", "US_SOCIAL_SECURITY_NUMBER", "PHONE_NUMBER"))
    assert (int(card[0]) & 0xFF, int(card[0]) >> 8, int(card[1]), skipset(card)) == (ord("#"), 0, 12, set(" -"))
    assert (int(ssn[0]) & 0xFF, int(ssn[0]) >> 8, int(ssn[1]), skipset(ssn)) == (ord("*"), 1, 4, set())
    import string
    assert (int(phone[0]) & 0xFF, int(phone[0]) >> 8, int(phone[1]), skipset(phone)) == (
        ord("*"), 0, 0, set(string.punctuation))
    assert not m[names.index("EMAIL_ADDRESS")].any()


def test_first_listing_entry_wins_then_first_catch_all():
    comp = pkg("compiler")
    names = ["EMAIL_ADDRESS", "PHONE_NUMBER", "IP_ADDRESS"]
    cfg = {"deidentify_config": {"info_type_transformations": {"transformations": [
        {"primitive_transformation": {"redact_config": {}}},
        {"info_types": [{"name": "EMAIL_ADDRESS"}], "primitive_transformation": {"replace_config": {
            "new_value": {"string_value": "x"}}}},
        {"info_types": [{"name": "EMAIL_ADDRESS"}, {"name": "PHONE_NUMBER"}],
         "primitive_transformation": {"replace_with_info_type_config": {}}},
        {"primitive_transformation": {"character_mask_config": {}}}]}}}
    kinds = [t.kind for t in comp.parse_deidentify(cfg, names)]
    assert kinds == [comp.XF_REPLACE, comp.XF_INFO_TYPE, comp.XF_REDACT]
    assert [t.kind for t in comp.parse_deidentify({}, names)] == [comp.XF_INFO_TYPE] * 3


_CRYPTO = {"crypto_replace_ffx_fpe_config": {"common_alphabet": "NUMERIC"}}
REJECTED = [
    ([{"primitive_transformation": _CRYPTO}], "crypto_replace_ffx_fpe_config"),
    ([{"primitive_transformation": {"date_shift_config": {"upper_bound_days": 3}}}], "date_shift_config"),
    ([{"primitive_transformation": {"bucketing_config": {}}}], "bucketing_config"),
    ([{"primitive_transformation": {"redact_config": {}, "replace_with_info_type_config": {}}}], "redact_config"),
    ([{"primitive_transformation": X._mask(masking_character="é")}], "masking_character"),
    ([{"primitive_transformation": X._mask(masking_character="**")}], "masking_character"),
    ([{"primitive_transformation": X._mask(characters_to_ignore=[{"characters_to_skip": "-ñ"}])}],
     "characters_to_skip"),
    ([{"primitive_transformation": X._mask(characters_to_ignore=[{"common_characters_to_ignore": "EMOJI"}])}],
     "EMOJI"),
    ([{"primitive_transformation": X._mask(number_to_mask=-1)}], "number_to_mask"),
    ([{"primitive_transformation": X._mask(number_to_mask="12")}], "number_to_mask '12'"),
    ([{"primitive_transformation": X._mask(reverse_order="false")}], "reverse_order"),
    ([{"info_types": [{"name": "NO_SUCH_TYPE"}], "primitive_transformation": {"redact_config": {}}}], "NO_SUCH_TYPE"),
    ([{"primitive_transformation": {"replace_config": {"new_value": {"string_value": "x" * 256}}}}], "256"),
    ([{"primitive_transformation": {"replace_config": {"new_value": {"integer_value": 3}}}}], "string_value"),
]


@pytest.mark.parametrize("transformations,word", REJECTED, ids=[w for _, w in REJECTED])
def test_rejected_forms_name_the_problem(transformations, word):
    comp = pkg("compiler")
    cfg = X.with_block(transformations)
    with pytest.raises(comp.RuleError, match=re.escape(word)):
        comp.parse_deidentify(cfg, ["EMAIL_ADDRESS", "PHONE_NUMBER"])


def test_record_transformations_rejected_and_limits_accepted():
    comp = pkg("compiler")
    cfg = copy.deepcopy(X.with_block(X.A))
    cfg["deidentify_config"]["record_transformations"] = {"field_transformations": []}
    with pytest.raises(comp.RuleError, match="record_transformations"):
        comp.parse_deidentify(cfg, ["EMAIL_ADDRESS"])
    ok = [{"primitive_transformation": {"replace_config": {"new_value": {"string_value": "é" * 127 + "x"}}}}]
    (t,) = comp.parse_deidentify(X.with_block(ok), ["EMAIL_ADDRESS"])
    assert t.kind == comp.XF_REPLACE and len(t.value) == 255
    (t,) = comp.parse_deidentify(X.with_block([{"primitive_transformation": {"replace_config": {
        "new_value": {"string_value": ""}}}}]), ["EMAIL_ADDRESS"])
    assert t.kind == comp.XF_REPLACE and t.value == b""


def test_reference_reproduces_the_known_answers(oracle_cfg):
    from oracle import pii_oracle as O
    cfg = X.with_block(X.A)
    names = oracle_cfg.type_names
    for text, want in X.KNOWN_A:
        fs = O.find_pii(text, oracle_cfg)
        assert xform_ref.apply_transform(text, fs, names, cfg) == want, text
    fs = O.find_pii(X.KNOWN_A[0][0], oracle_cfg)
    assert [(f.start, f.end) for f in fs] == [(10, 21), (21, 28)]
    fs = O.find_pii(X.KNOWN_A[-1][0], oracle_cfg)
    assert [names[f.type_id] for f in fs] == ["IP_ADDRESS"]
    pn = names.index("PERSON_NAME")
    for prim, want in X.KNOWN_EXT:
        cfg = X.with_block([{"info_types": [{"name": "PERSON_NAME"}], "primitive_transformation": prim}])
        fs = O.find_pii(X.EXT_TEXT, oracle_cfg, extra=[(X.EXT_SPAN[0], X.EXT_SPAN[1], pn, 4)])
        assert [(f.start, f.end, f.type_id) for f in fs] == [(X.EXT_SPAN[0], X.EXT_SPAN[1], pn)]
        assert xform_ref.apply_transform(X.EXT_TEXT, fs, names, cfg) == want
    # the shipped block and no block: the oracle's own "[TYPE]" redaction
    for text, _ in X.KNOWN_A:
        red, fs = O.redact(text, oracle_cfg)
        assert xform_ref.apply_transform(text, fs, names, X.shipped()) == red
        assert xform_ref.apply_transform(text, fs, names, {}) == red


def test_long_name_rows_hold_what_the_gpu_tests_take_them_for(oracle_cfg):
    """X.long_rows / X.LONG_MASKS: the only finding is the candidate, code points of every length straddle
    the 16-byte window edges of both walk directions, and the two counts end where their names say"""
    from oracle import pii_oracle as O
    name, L = X.LONG_NAME, len(X.LONG_NAME)
    chars = name.decode()
    at = np.cumsum([0] + [len(c.encode()) for c in chars])           # code point k = bytes at[k] .. at[k + 1]
    assert L == 68 and {int(b - a) for a, b in zip(at, at[1:])} == {1, 2, 3, 4} and " " in chars and "-" in chars
    for edge in (16, 32, L - 16, L - 32, L - 48):
        assert edge not in at, edge
    texts, spans = X.long_rows()
    pn = oracle_cfg.type_names.index("PERSON_NAME")
    assert [len(t) for t in texts] == [96] * 16 and [s for s, _ in spans] == list(range(16))
    for t, (s, e) in zip(texts, spans):
        assert t[s:e] == name and not O.find_pii(t, oracle_cfg)
        fs = O.find_pii(t, oracle_cfg, extra=[(s, e, pn, 4)])
        assert [(f.start, f.end, f.type_id) for f in fs] == [(s, e, pn)]
    star = lambda k: b"*" * int(at[k + 1] - at[k])                   # noqa: E731
    fwd = xform_ref.mask(name, X.LONG_MASKS["forward_18"]["character_mask_config"])
    assert fwd == b"#" * int(at[18]) + name[at[18]:] and 16 <= at[17] < at[18] < 32
    rev = xform_ref.mask(name, X.LONG_MASKS["reverse_21"]["character_mask_config"])
    kept = [k for k in range(len(chars) - 1, -1, -1) if chars[k] not in " -"][21:]
    assert rev == b"".join(chars[k].encode() if k in kept or chars[k] in " -" else star(k) for k in range(len(chars)))
    last, stop = [k for k in range(len(chars)) if chars[k] not in " -" and k not in kept][0], kept[0]
    assert L - 48 <= at[stop] < at[last] < L - 32                    # the third window from the end
    assert xform_ref.mask(name, X.LONG_MASKS["forward_all"]["character_mask_config"]) == b"*" * L
    assert xform_ref.mask(name, X.LONG_MASKS["reverse_all"]["character_mask_config"]) == b"*" * L


def test_header_declares_and_library_exports_type_transform():
    E = pkg("engine")
    src = open(os.path.join(ROOT, "include", "pii_engine.h")).read()
    assert re.search(r"^int\s+pii_type_transform\s*\(\s*struct pii_engine\*\s*\w+,\s*uint32_t\s+\w+\)", src, re.M)
    for i, name in enumerate(("INFO_TYPE", "REPLACE", "REDACT", "MASK", "KEEP")):
        assert re.search(rf"^#define PII_XF_{name} {i}$", src, re.M)
        assert getattr(E, "PII_XF_" + name) == i == getattr(pkg("compiler"), "XF_" + name)
    assert "pii_type_transform" in E.EXPORTS
    assert hasattr(E.load_library(), "pii_type_transform")
    assert hasattr(E.Engine, "type_transform")


def test_service_takes_a_dlp_config_path():
    import inspect
    S = pkg("service")
    assert "dlp_config_path" in inspect.signature(S.PiiService.__init__).parameters
    with pytest.raises(ValueError):
        S.PiiService(engine=object(), dlp_config_path="x.json")
