"""General exclusion rules in the rule compiler: PARTIAL_MATCH, more excluder patterns than k_select's
streaming form keeps, a type both excluded and excluding.  Such a rule set compiles to var.xg_* / det.xgidx
beside empty streaming lists; every other rule set compiles to the bytes it always did."""
import hashlib
import json
import os
import re

import numpy as np
import pytest
import yaml

import excl_configs as XC
from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def builtin():
    with open(os.path.join(pkg("compiler").RULES_DIR, "builtin_infotypes.yaml")) as f:
        return yaml.safe_load(f)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "excl_blob_sha256.json")) as f:
        return json.load(f)


def _compile(cfg, builtin):
    comp = pkg("compiler")
    return comp.compile_rules(comp.Rules(cfg, builtin))


def _lists(c):
    """(variant, type name) -> [(excluder type name, partial)] of a general blob"""
    comp, S, names = pkg("compiler"), c.sections, c.rules.type_names
    T = len(names)
    off, ids = S["var.xg_off"], S["var.xg_ids"]
    out = {}
    for k in range(len(off) - 1):
        if off[k + 1] > off[k]:
            out[(k // T, names[k % T])] = [(names[int(i) & ~comp.XG_PARTIAL], bool(int(i) & comp.XG_PARTIAL))
                                           for i in ids[off[k]:off[k + 1]]]
    return out


def _assert_general(c):
    comp, S = pkg("compiler"), c.sections
    P, T, V = int(S["meta"][0]), int(S["meta"][2]), int(S["meta"][3])
    assert S["var.xg_off"].dtype == np.uint32 and S["var.xg_off"].shape == (V * T + 1,)
    assert S["var.xg_ids"].dtype == np.uint16 and len(S["var.xg_ids"]) >= int(S["var.xg_off"][-1]) > 0
    assert S["det.xgidx"].dtype == np.uint8 and S["det.xgidx"].shape == (P,)
    idx = sorted(int(x) for x in S["det.xgidx"] if x != 0xFF)
    assert idx == list(range(len(idx))) and 0 < len(idx) <= comp.NX_MAX
    # the streaming lists are empty and no window re-scan runs incrementally
    assert not S["var.excl_off"].any() and (S["det.exidx"] == 0xFF).all()
    assert int(S["meta"][13]) == 0
    return idx


def test_partial_match_compiles(builtin):
    """(fails before general exclusion rules: PARTIAL_MATCH was a RuleError)"""
    c = _compile(XC.g1(), builtin)
    idx = _assert_general(c)
    assert len(idx) == 5                         # EMAIL_ADDRESS (the shipped handle rule) + the four custom types
    lists = _lists(c)
    V = int(c.sections["meta"][3])
    for v in range(V):                           # the rules are in every context variant
        assert lists[(v, "EMAIL_ADDRESS")] == [("OUR_DOMAIN", True)]
        assert lists[(v, "PHONE_NUMBER")] == [("TAIL_REF", True)]
        assert lists[(v, "US_SOCIAL_SECURITY_NUMBER")] == [("PAIR3", True)]
        assert lists[(v, "CREDIT_CARD_NUMBER")] == [("TEST_CARD", False)]
        assert lists[(v, "SOCIAL_HANDLE")] == [("EMAIL_ADDRESS", False)]
    # excluder patterns are the patterns of the listed types
    S = c.sections
    named = {n for l in lists.values() for n, _ in l}
    for p in c.rules.patterns:
        assert (S["det.xgidx"][p.pid] != 0xFF) == (p.type_name in named)


def test_many_full_match_excluders_compile(builtin):
    c = _compile(XC.g2(), builtin)
    assert len(_assert_general(c)) == 5 > pkg("compiler").NE_MAX
    assert not any(partial for l in _lists(c).values() for _, partial in l)


def test_allow_list_with_transformations_compiles(builtin):
    comp = pkg("compiler")
    c = _compile(XC.g3(), builtin)
    _assert_general(c)
    kinds = dict(zip(c.rules.type_names, c.sections["xf.kind"]))
    assert all(kinds[n] == comp.XF_KEEP for n in XC.CUSTOM_NAMES)
    assert all(kinds[n] == comp.XF_INFO_TYPE for n in XC.BUILTIN_LISTED)


def test_excluded_and_excluding_type_is_general(builtin):
    """EMAIL_ADDRESS excludes handles in the shipped rules; a FULL_MATCH rule on it alone makes the set general"""
    c = _compile(XC.with_custom([XC.excl_rule("EMAIL_ADDRESS", "OUR_DOMAIN", XC.FULL)], custom=XC.CUSTOM[:1]), builtin)
    assert len(_assert_general(c)) == 2


def _sha(blob):
    return hashlib.sha256(blob).hexdigest()


def test_shipped_blob_unchanged(compiled, golden):
    assert _sha(compiled.blob) == golden["shipped"]
    assert "var.xg_off" not in compiled.sections and int(compiled.sections["meta"][13]) == 1


def test_context_variant_blob_unchanged(golden):
    comp = pkg("compiler")
    c = comp.compile_default(os.path.join(comp.RULES_DIR, "context_variant.json"))
    assert _sha(c.blob) == golden["context_variant"]


def test_config5_blob_unchanged(golden, tmp_path):
    comp, G = pkg("compiler"), pkg("rulegen")
    path = str(tmp_path / "config5.json")
    G.Config5().save(path)
    assert _sha(comp.compile_rules(comp.Rules.load(path)).blob) == golden["config5"]


def test_two_excluder_patterns_stay_streaming(builtin):
    c = _compile(XC.one_more_full(), builtin)
    S = c.sections
    assert not any(k in S for k in ("var.xg_off", "var.xg_ids", "det.xgidx"))
    assert sorted(int(x) for x in S["det.exidx"] if x != 0xFF) == [0, 1]
    assert int(S["var.excl_off"][-1]) > 0 and int(S["meta"][13]) == 1


def test_limits_mirror_the_engine():
    comp = pkg("compiler")
    with open(os.path.join(ROOT, "context-based-pii_amd", "csrc", "pii_layout.h")) as f:
        src = f.read()
    for name in ("NE_MAX", "NX_MAX"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, name
        assert int(m.group(1)) == getattr(comp, name), name
    m = re.search(r"constexpr\s+uint16_t\s+XG_PARTIAL\s*=\s*(0x[0-9a-fA-F]+)\s*;", src)
    assert m and int(m.group(1), 16) == comp.XG_PARTIAL
    assert comp.NX_MAX >= 64


def _rule(ex):
    return XC.with_custom([{"info_types": [{"name": "EMAIL_ADDRESS"}], "rules": [{"exclusion_rule": ex}]}])


@pytest.mark.parametrize("form, body", [
    ("regex", {"pattern": "@acme"}),
    ("dictionary", {"word_list": {"words": ["acme"]}}),
    ("exclude_by_hotword", {"hotword_regex": {"pattern": "test"}, "proximity": {"window_before": 10}}),
])
def test_other_exclusion_forms_are_refused(form, body, builtin):
    comp = pkg("compiler")
    with pytest.raises(comp.RuleError, match=r"exclusion_rule\.%s is not supported" % form):
        _compile(_rule({form: body, "matching_type": XC.PARTIAL}), builtin)


def test_unknown_matching_type_is_refused(builtin):
    comp = pkg("compiler")
    ex = {"exclude_info_types": {"info_types": [{"name": "OUR_DOMAIN"}]}, "matching_type": "MATCHING_TYPE_INVERSE_MATCH"}
    with pytest.raises(comp.RuleError, match="unknown matching_type MATCHING_TYPE_INVERSE_MATCH"):
        _compile(_rule(ex), builtin)


def test_too_many_excluder_patterns_are_refused(builtin):
    comp = pkg("compiler")
    n = comp.NX_MAX + 1
    custom = [("ALLOW_%02d" % i, "zq%02dx" % i) for i in range(n)]
    rules = [{"info_types": [{"name": "PHONE_NUMBER"}], "rules": [{"exclusion_rule": {
        "exclude_info_types": {"info_types": [{"name": name} for name, _ in custom]}, "matching_type": XC.PARTIAL}}]}]
    cfg = XC.with_custom(rules, custom=custom)
    cfg["inspect_config"]["rule_set"] = rules         # (without the shipped handle rule: exactly n excluder patterns)
    with pytest.raises(comp.RuleError, match=r"%d excluder patterns \(more than %d\)" % (n, comp.NX_MAX)):
        _compile(cfg, builtin)


def test_external_type_in_an_exclusion_rule_is_refused(builtin):
    comp = pkg("compiler")
    ext = builtin["external_types"][0]
    for victim, excluder in (("EMAIL_ADDRESS", ext), (ext, "OUR_DOMAIN")):
        with pytest.raises(comp.RuleError, match="external type %s cannot be named" % ext):
            _compile(XC.with_custom([XC.excl_rule(victim, excluder, XC.PARTIAL)]), builtin)
